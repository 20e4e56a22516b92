"""GPU: the decode hand-offs' row sums (t2s_persist1.hip gather_halves: both row halves of a
granule column summed by one wave, the partial sums passed by a lane swap) bit for bit
against tests/golden/handoff_halves.npz -- what k_decode_persist1 computed, with the halves in
two waves and the sums passed through LDS, before the change (tools/record_handoff_fixture.py).

The gather always covers the 512 columns, so the smallest prompt serves: R = 12, S = 10,
H = 41 (N0 = 42), 9 forced steps -- every slot of the 4-deep granule ring twice, one 64-key
attention round.  Layer 23's K/V rows after nine steps depend on every sum of both hops in
every layer and step.  Cases: B = 1 on the whole chip; a two-sentence stream on two decode
lanes of 3 groups beside 64 vocoder CUs; B = 3 through k_decode_persist1m; one *_each launch."""
import hashlib
import os

import numpy as np
import pytest

from tests.common import character, t2s_inputs

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handoff_halves.npz")
R_, S_, H_, STEPS, TAG = 12, 10, 41, 9, "p12"
N0 = R_ + S_ + H_ // 2
ROWS = N0 + STEPS
LAYERS = (0, 11, 23)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    assert int(g["kv_rows"]) == ROWS
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def eng():
    from genie_tts_amd.engine import Engine
    w = character("v2")
    e = Engine({"t2s_encoder": w["t2s_encoder"], "t2s": w["t2s"]}, "v2")
    e.set_option("persist", 1)
    yield e
    e.set_vocoder_cus(0)
    e.close()


def sentence():
    return t2s_inputs(R=R_, S=S_, H=H_, tag=TAG)


def sampler(greedy):
    from genie_tts_amd.engine import make_sampler
    if greedy:
        return make_sampler(force_steps=STEPS)
    return make_sampler(top_k=5, greedy=False, seed=1234, force_steps=STEPS)


def want_tokens(gold, greedy):
    return gold["tokens_greedy" if greedy else "tokens_sampled"].tolist()


def read_kv(eng, layer, seq=0):
    return tuple(t.cpu().numpy() for t in eng.t2s_read_kv(layer, seq))


def _launches(eng):
    return [eng.counter(n) for n in ("persist_launches", "persist_timeouts", "persist1_f16_reruns")]


@pytest.mark.parametrize("greedy", [True, False])
def test_single_sequence_whole_chip(eng, gold, greedy):
    eng.set_vocoder_cus(0)
    c0 = _launches(eng)
    tok = eng.t2s_generate([sentence()], sampler(greedy))[0].tolist()
    assert _launches(eng) == [c0[0] + 1, c0[1], c0[2]]   # one persistent launch, completed
    assert tok == want_tokens(gold, greedy)
    sha = gold["sha_greedy" if greedy else "sha_sampled"]
    for layer in range(24):
        k, v = read_kv(eng, layer)
        assert k.shape == v.shape == (ROWS, 512)
        got = (hashlib.sha256(k.tobytes()).hexdigest(), hashlib.sha256(v.tobytes()).hexdigest())
        assert got == tuple(sha[layer]), f"layer {layer}"
        if greedy and layer in LAYERS:
            assert np.array_equal(k, gold[f"k{layer}"]) and np.array_equal(v, gold[f"v{layer}"]), f"layer {layer}"


@pytest.mark.parametrize("greedy", [True, False])
def test_two_sentence_stream_on_two_lanes(eng, gold, greedy):
    """vocoder_cus = 64 leaves 192 decode CUs: two lanes of 3 groups, lane 1 on its own ring."""
    utts = [sentence(), sentence()]   # two tuple objects (a prefetch is matched by identity)
    sp = sampler(greedy)
    eng.set_vocoder_cus(64)
    try:
        t0 = eng.counter("persist_timeouts")
        eng.t2s_prefetch(utts[1], sp)
        eng.t2s_generate_start(utts[0], sp)
        eng.t2s_generate_start(utts[1], sp)
        got = [eng.t2s_generate_finish().tolist(), eng.t2s_generate_finish().tolist()]
        assert eng.counter("persist_timeouts") == t0
    finally:
        eng.set_vocoder_cus(0)
    assert got == [want_tokens(gold, greedy)] * 2


def test_three_sequences_multi_kernel(eng, gold):
    """k_decode_persist1m at B = 3: the fixture's sentence in slot 0 beside two ragged ones."""
    eng.set_vocoder_cus(0)
    utts = [sentence(), t2s_inputs(R=15, S=13, H=52, tag="hh1"), t2s_inputs(R=9, S=7, H=30, tag="hh2")]
    c0 = _launches(eng)
    tok = [t.tolist() for t in eng.t2s_generate(utts, sampler(True))]
    assert _launches(eng) == [c0[0] + 1, c0[1], c0[2]]
    kv = [read_kv(eng, 23, seq=b) for b in range(3)]
    assert tok[0] == want_tokens(gold, True)
    assert np.array_equal(kv[0][0], gold["k23"]) and np.array_equal(kv[0][1], gold["v23"])
    for b in range(3):
        alone = eng.t2s_generate([utts[b]], sampler(True))[0].tolist()
        k, v = read_kv(eng, 23)
        assert tok[b] == alone, f"sequence {b}"
        assert k.shape == kv[b][0].shape and k.shape[0] > STEPS
        assert np.array_equal(k, kv[b][0]) and np.array_equal(v, kv[b][1]), f"sequence {b}"
    # slot 0 draws the noise of a B = 1 generate: the sampler path's hand-off (form_u(24))
    assert eng.t2s_generate(utts, sampler(False))[0].tolist() == want_tokens(gold, False)


@pytest.mark.parametrize("greedy", [True, False])
def test_each_launch(eng, gold, greedy):
    """A per-sequence sampler table at B = 1: k_decode_persist1_each."""
    eng.set_vocoder_cus(0)
    c0 = _launches(eng)
    tok = eng.t2s_generate([sentence()], samplers=[sampler(greedy)], streams=[0])[0].tolist()
    assert _launches(eng) == [c0[0] + 1, c0[1], c0[2]]
    assert tok == want_tokens(gold, greedy)
    k, v = read_kv(eng, 23)
    if greedy:
        assert np.array_equal(k, gold["k23"]) and np.array_equal(v, gold["v23"])
