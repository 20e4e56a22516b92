"""GPU: the single-sequence persistent decode (t2s_persist1.hip) where a launch is abandoned, and
its stamped variant.

Abandoned launches.  A launch that meets the fp16 limit of its split MFMA operands sets the error
word, raises the workgroup's fail flag and every workgroup leaves at its next barrier or wait.  It
must leave no trace: no sequence state written back, no granule of this step with garbage behind
its tag, the re-run (per-step graphs) starting from an untouched state -- wherever in a layer the
flag is tested (between a hop's barrier and the first store that leaves the workgroup there is
room to move that test; this is the guard for doing so).  The test hook persist1_f16_limit = 1, 2, 4,
... lowers the limit until it no longer trips, on the smallest utterance the encoder takes
(4 reference phones, 4 text phones, 8 SSL frames: N0 = 12 keys, 6 forced steps, greedy).  With the
synthetic character's default weight seed the largest split operand of these 6 steps lies in
[4, 8): limits 1, 2 and 4 trip (at different hops: the first operand past 1 is not the first past
4), 8 does not -- the test asserts at least three trips and the one clean launch, so another seed
that moves the maximum out of [4, 2^16) fails it loudly.  A launch that trips is re-run on the
per-step graphs, a clean one is the persistent kernel's own result, whose K/V rows differ from the
graphs' in the last bits: the K/V yardstick is therefore what the parent commit left after the
same calls, tests/golden/decode_abandon.json (SHA-256 of the K and V rows of layers 0, 11 and 23
after every call; tools/record_decode_abandon_fixture.py runs abandon_calls below on the commit
whose behaviour is the reference).  No hand-off timeout is forced here.

The trace variant.  Option "ptrace" launches k_decode_persist1_trace (the stamps are compiled out
of k_decode_persist1): same tokens, stamps of a layer-12 attention workgroup non-zero and in
program order; with the option off the product kernel runs (it is given no stamp buffer: the
engine frees it with the option, so what can be seen is that the next buffer starts out zero, the
tokens stay and no counter moves)."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.common import character, t2s_inputs

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_abandon.json")
R_, S_, H_, STEPS = 4, 4, 8, 6
LAYERS = (0, 11, 23)
COUNTERS = ("persist1_f16_reruns", "persist_timeouts")


def sentence(tag="ab0"):
    return t2s_inputs(R=R_, S=S_, H=H_, tag=tag)


def kv_sha(eng):
    out = {}
    for layer in LAYERS:
        k, v = (t.cpu().numpy() for t in eng.t2s_read_kv(layer, 0))
        out[str(layer)] = [hashlib.sha256(k.tobytes()).hexdigest(), hashlib.sha256(v.tobytes()).hexdigest(),
                           int(k.shape[0])]
    return out


def abandon_calls(eng, lanes):
    """The calls of the abandon test on an engine with persist = 1: the limit doubled from 1 until a
    launch no longer trips, then one generate with the limit back at 0.  lanes: every generate as two
    started generates side by side (vocoder_cus = 64: two decode lanes), else one t2s_generate.
    Returns {"graphs": tokens with persist = 0, "calls": [{limit, tripped, tokens, kv}], "after":
    {tokens, kv}, "timeouts": persist_timeouts risen}; tokens: one list per sentence."""
    from genie_tts_amd.engine import make_sampler
    sp = make_sampler(force_steps=STEPS)
    utts = [sentence("ab0"), sentence("ab1")] if lanes else [sentence("ab0")]

    def generate():
        if not lanes:
            return [eng.t2s_generate(utts, sp)[0].tolist()]
        for u in utts:
            eng.t2s_generate_start(u, sp)
        return [eng.t2s_generate_finish().tolist() for _ in utts]

    eng.set_vocoder_cus(64 if lanes else 0)
    try:
        eng.set_option("persist", 0)
        graphs = [eng.t2s_generate([u], sp)[0].tolist() for u in utts]
        eng.set_option("persist", 1)
        t0 = eng.counter("persist_timeouts")
        calls, limit = [], 1
        while True:
            r0 = eng.counter("persist1_f16_reruns")
            eng.set_option("persist1_f16_limit", limit)
            try:
                tok = generate()
            finally:
                eng.set_option("persist1_f16_limit", 0)
            tripped = eng.counter("persist1_f16_reruns") - r0
            calls.append({"limit": limit, "tripped": int(tripped), "tokens": tok, "kv": kv_sha(eng)})
            if not tripped or limit >= 65536:
                break
            limit *= 2
        r0 = eng.counter("persist1_f16_reruns")
        after = {"tokens": generate(), "kv": kv_sha(eng), "tripped": int(eng.counter("persist1_f16_reruns") - r0)}
        return {"graphs": graphs, "calls": calls, "after": after,
                "timeouts": int(eng.counter("persist_timeouts") - t0)}
    finally:
        eng.set_vocoder_cus(0)


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def eng():
    from genie_tts_amd.engine import Engine
    w = character("v2")
    e = Engine({"t2s_encoder": w["t2s_encoder"], "t2s": w["t2s"]}, "v2")
    e.set_option("persist", 1)
    yield e
    e.set_vocoder_cus(0)
    e.close()


@pytest.mark.parametrize("lanes", [False, True], ids=["whole_chip", "two_lanes"])
def test_abandoned_launch_leaves_no_trace(eng, gold, lanes):
    got = abandon_calls(eng, lanes)
    want = gold["two_lanes" if lanes else "whole_chip"]
    n = len(got["graphs"])
    trips = [c for c in got["calls"] if c["tripped"]]
    print("limits", [(c["limit"], c["tripped"]) for c in got["calls"]])
    assert len(trips) >= 3 and not got["calls"][-1]["tripped"], [(c["limit"], c["tripped"]) for c in got["calls"]]
    assert all(c["tripped"] >= n for c in trips)   # every launch in flight met the limit
    for c in got["calls"]:
        assert c["tokens"] == got["graphs"], c["limit"]
    assert got["after"]["tokens"] == got["graphs"] and got["after"]["tripped"] == 0
    assert got["timeouts"] == 0
    # what the parent commit left after the same calls
    assert [(c["limit"], c["tripped"]) for c in got["calls"]] == [(c["limit"], c["tripped"]) for c in want["calls"]]
    assert got["graphs"] == want["graphs"]
    for c, w in zip(got["calls"], want["calls"]):
        assert c["kv"] == w["kv"], c["limit"]
    assert got["after"]["kv"] == want["after"]["kv"]


def test_trace_variant(eng):
    from genie_tts_amd.engine import make_sampler
    sp = make_sampler(force_steps=10)   # the probe reads step 8 and step 9's layer 0
    utt = sentence("tr0")
    eng.set_vocoder_cus(0)
    c0 = [eng.counter(n) for n in COUNTERS]
    plain = eng.t2s_generate([utt], sp)[0].tolist()
    eng.set_option("ptrace", 1)
    try:
        assert not eng.ptrace().any()   # a fresh buffer
        traced = eng.t2s_generate([utt], sp)[0].tolist()
        tr = eng.ptrace().astype(np.int64)
    finally:
        eng.set_option("ptrace", 0)
    assert traced == plain
    # 8 layer groups: layer 12 is group 4's, attention workgroups 128..143; stamps in program order
    # (0 before the x_l wait, 1 x_l, 6 q/k/v, 7 K/V landed, 2 barrier, 3 softmax, 4 head output, 5 published)
    for wg in (128, 135, 143):
        st = tr[wg, [0, 1, 6, 7, 2, 3, 4, 5]]
        assert (st > 0).all() and (np.diff(st) >= 0).all(), (wg, st.tolist())
        assert st[-1] - st[0] < 100 * 1000   # one layer: far below 1 ms of 100 MHz ticks
    # the option off again: the product kernel, which holds no stamp code
    again = eng.t2s_generate([utt], sp)[0].tolist()
    eng.set_option("ptrace", 1)
    try:
        assert not eng.ptrace().any()   # nothing of the untraced launch in the next stamp buffer
    finally:
        eng.set_option("ptrace", 0)
    assert again == plain
    assert [eng.counter(n) for n in COUNTERS] == c0
