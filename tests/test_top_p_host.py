"""Host (no GPU): nucleus sampling (top_p) above the engine -- the Sampler struct against the
C header, make_sampler / api / server validation, the server's per-sampler rounds, and the
oracle helper (tests/top_p_oracle.py) against a brute-force float64 loop.
"""
import asyncio
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import top_p_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the struct and make_sampler
def test_make_sampler_top_p():
    from genie_tts_amd.engine import make_sampler
    assert make_sampler(top_p=0.8).top_p == pytest.approx(0.8)
    assert make_sampler().top_p == 1.0
    sp = make_sampler(5, 0.7, 1.2, False, 9, 100, 3)              # the positional order is as before
    assert (sp.top_k, sp.greedy, sp.seed, sp.max_steps, sp.force_steps, sp.top_p) == (5, 0, 9, 100, 3, 1.0)
    for bad in (0.0, -0.1, 1.5, math.nan, math.inf):
        with pytest.raises(ValueError):
            make_sampler(top_p=bad)


def test_sampler_struct_matches_the_c_header(tmp_path):
    from genie_tts_amd.engine import Sampler
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "genie_engine.h"\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(gsv_sampler), offsetof(gsv_sampler, top_p),\n'
                   '           offsetof(gsv_sampler, seed), offsetof(gsv_sampler, force_steps));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_p, off_seed, off_force = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                               text=True).stdout.split())
    assert ctypes.sizeof(Sampler) == size
    assert Sampler.top_p.offset == off_p
    assert (Sampler.seed.offset, Sampler.force_steps.offset) == (off_seed, off_force) == (16, 28)   # as before


# ------------------------------------------------------------------ api
def test_api_rejects_bad_sampling_before_touching_a_model(monkeypatch):
    from genie_tts_amd import api

    def boom(*a, **k):
        raise AssertionError("a model was touched")
    monkeypatch.setattr(api.model_manager, "get", boom)
    monkeypatch.setattr(api, "_synthesize_all", boom)
    monkeypatch.setattr(api, "_synthesize", boom)
    monkeypatch.setitem(api._reference_audios, "c", object())
    txt = np.array([3, 5, 7], np.int64)
    bads = [dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(top_p=math.nan), dict(top_k=0), dict(top_k=65),
            dict(top_k=2.5), dict(temperature=0.0), dict(temperature=math.inf), dict(repetition_penalty=-1.0),
            dict(seed=-1), dict(seed=1 << 64)]
    for bad in bads:
        with pytest.raises(ValueError):
            api.tts("c", txt, **bad)

        async def go():
            return [c async for c in api.tts_async("c", "x", **bad)]
        with pytest.raises(ValueError):
            asyncio.run(go())


def test_api_keywords_override_a_copy_of_the_base_sampler(monkeypatch):
    from types import SimpleNamespace
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler, sampler_key
    own = make_sampler(top_k=7, greedy=False, seed=3)
    m = SimpleNamespace(T2S_FIRST_STAGE_DECODER=SimpleNamespace(sampler=own))
    monkeypatch.setattr(api.model_manager, "get", lambda name: m)
    monkeypatch.setitem(api._reference_audios, "c", object())
    seen = []
    monkeypatch.setattr(api, "_synthesize_all", lambda name, sents, tb, sampler, **kw: seen.append(sampler) or [])
    txt = np.array([3, 5, 7], np.int64)
    api.tts("c", txt)
    assert seen[-1] is None                                        # no keyword: today's call, untouched
    api.tts("c", txt, top_p=0.8, seed=11)
    sp = seen[-1]
    assert sp is not own and (sp.top_k, sp.seed, sp.greedy) == (7, 11, 0) and sp.top_p == pytest.approx(0.8)
    assert own.top_p == 1.0 and own.seed == 3                      # the character's sampler is not modified
    base = make_sampler(top_k=20, greedy=False, temperature=0.5)
    api.tts("c", txt, sampler=base, top_k=9)
    sp = seen[-1]
    assert (sp.top_k, sp.temperature) == (9, 0.5) and base.top_k == 20
    api.tts("c", txt, sampler=base)
    assert seen[-1] is base
    assert sampler_key(make_sampler()) != sampler_key(make_sampler(top_p=0.5))
    zero = make_sampler()
    zero.top_p = 0.0
    assert sampler_key(zero) == sampler_key(make_sampler())        # 0 reads as 1


def test_tts_async_passes_the_sampler_through(monkeypatch):
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    monkeypatch.setitem(api._reference_audios, "c", object())
    got = []
    monkeypatch.setattr(api, "_synthesize",
                        lambda name, s, text_bert=None, sampler=None, speed=1.0: got.append(sampler))
    base = make_sampler(greedy=False, top_p=0.7)

    async def go(**kw):
        return [c async for c in api.tts_async("c", "x", **kw)]
    asyncio.run(go(sampler=base))
    assert got[-1] is base
    asyncio.run(go(sampler=base, top_p=0.4))
    assert got[-1] is not base and got[-1].top_p == pytest.approx(0.4) and base.top_p == pytest.approx(0.7)
    asyncio.run(go())
    assert got[-1] is None


# ------------------------------------------------------------------ the server
def _worker(monkeypatch, own=None, gate=None):
    """_worker_main on a thread over stubs, as tests/test_speed_host.py drives it; returns
    (parent pipe, thread, the samplers each round's generate got with its batch size)."""
    import multiprocessing as mp
    import threading
    from genie_tts_amd import api
    from genie_tts_amd.inference import tts_client
    from genie_tts_amd.model_manager import model_manager
    from genie_tts_amd.server import _worker_main

    class M:
        LANGUAGE = "Japanese"
        ENGINE = None
        VITS = None
        T2S_FIRST_STAGE_DECODER = type("D", (), {"sampler": own})()

    rounds = []

    def t2s(items, ref, m, sp):
        if gate is not None:
            assert gate.wait(60)                   # holds the first round until the test has sent its burst
        rounds.append((len(items), sp))
        return [None] * len(items)
    model = M()
    monkeypatch.setattr(model_manager, "get", lambda name: model)
    monkeypatch.setitem(api._reference_audios, "a", object())
    monkeypatch.setattr(tts_client, "tts_batch_t2s", t2s)
    monkeypatch.setattr(tts_client, "tts_batch_vocoder",
                        lambda items, toks, ref, m, overlapped=False, speed=1.0: [np.zeros(640, np.float32)] * len(items))
    parent, child = mp.Pipe()
    t = threading.Thread(target=_worker_main, args=(0, child, {"g2p": "genie_tts_amd.stubs:toy_g2p"}), daemon=True)
    t.start()
    assert parent.poll(60) and parent.recv()["kind"] == "ready"
    return parent, t, rounds


def _collect(parent, ids):
    out = {i: [] for i in ids}
    open_ = set(ids)
    while open_:
        assert parent.poll(60), "worker did not answer"
        m = parent.recv()
        if m["id"] in out:
            out[m["id"]].append(m["kind"] if m["kind"] != "error" else ("error", m["detail"]))
            if m["kind"] in ("end", "error"):
                open_.discard(m["id"])
    return out


def test_worker_rejects_a_bad_top_p_for_that_request_only(monkeypatch):
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    own = make_sampler(greedy=False, seed=1)
    parent, t, rounds = _worker(monkeypatch, own)
    try:
        parent.send(dict(cmd="tts", id=1, character_name="a", text="かき。", top_p=1.5))
        got = _collect(parent, [1])[1]
        assert len(got) == 1 and got[0][0] == "error" and got[0][1].startswith("sampling:") and "top_p" in got[0][1]
        assert rounds == []
        parent.send(dict(cmd="tts", id=2, character_name="a", text="かき。", top_p=0.8))
        assert _collect(parent, [2])[2] == ["chunk", "end"]
        assert len(rounds) == 1 and rounds[0][1] is not own and rounds[0][1].top_p == pytest.approx(0.8)
        assert rounds[0][1].seed == 1 and own.top_p == 1.0
        parent.send(dict(cmd="tts", id=3, character_name="a", text="かき。"))      # no control: the character's own
        assert _collect(parent, [3])[3] == ["chunk", "end"]
        assert rounds[-1][1] is own
    finally:
        parent.send(None)
        t.join(timeout=30)
        api.set_g2p(None)


def test_rounds_group_by_sampler(monkeypatch):
    """Five requests pending at once (they arrive while a first round is held): the two with
    top_p 0.5 share a round, the one with 0.9 waits for the next, and a control equal to the
    character's own value batches with the request that gives none."""
    import threading
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    own = make_sampler(greedy=False, seed=1)
    gate = threading.Event()
    parent, t, rounds = _worker(monkeypatch, own, gate)
    try:
        parent.send(dict(cmd="tts", id=0, character_name="a", text="かき。"))
        for rid, kw in ((1, dict(top_p=0.5)), (2, dict(top_p=0.9)), (3, dict(top_p=0.5)), (4, {}),
                        (5, dict(top_k=own.top_k))):
            parent.send(dict(cmd="tts", id=rid, character_name="a", text="かき。", **kw))
        gate.set()
        got = _collect(parent, [0, 1, 2, 3, 4, 5])
        assert all(v == ["chunk", "end"] for v in got.values()), got
        # the burst may or may not have reached the worker before round 0 began: request 0 is
        # alone or with its equals (4, 5); what follows is one round per sampler, in arrival order
        sizes = [(n, round(float(sp.top_p), 3)) for n, sp in rounds]
        assert sizes in ([(1, 1.0), (2, 0.5), (1, 0.9), (2, 1.0)], [(3, 1.0), (2, 0.5), (1, 0.9)]), sizes
        assert rounds[1][1].top_k == own.top_k and rounds[1][1] is not own
    finally:
        parent.send(None)
        t.join(timeout=30)
        api.set_g2p(None)


def _echo_worker(index, conn, cfg):
    """A host-only worker: answers a tts request with the names of the sampling fields it got."""
    conn.send(dict(kind="ready", id=-1, index=index))
    while True:
        msg = conn.recv()
        if msg is None:
            return
        if msg["cmd"] == "tts":
            if msg.get("seed") == 400:         # stands in for the worker's own rejection
                conn.send(dict(kind="error", id=msg["id"], detail="sampling: refused"))
                continue
            keys = sorted(k for k in ("top_k", "top_p", "temperature", "repetition_penalty", "seed") if k in msg)
            conn.send(dict(kind="chunk", id=msg["id"], data=",".join(keys).encode()))
            conn.send(dict(kind="end", id=msg["id"]))
        else:
            conn.send(dict(kind="ok", id=msg["id"]))


def test_tts_payload_validates_the_sampling_fields():
    import httpx
    from genie_tts_amd.server import Router, create_app

    async def run():
        router = Router([0], worker=_echo_worker)
        router.start(asyncio.get_running_loop(), timeout=120)
        tr = httpx.ASGITransport(app=create_app(router))
        try:
            async with httpx.AsyncClient(transport=tr, base_url="http://t") as cl:
                r = await cl.post("/tts", json=dict(character_name="a", text="x"))
                assert r.status_code == 200 and r.content == b""          # absent fields are not sent on
                r = await cl.post("/tts", json=dict(character_name="a", text="x", top_p=0.8, top_k=5, seed=3))
                assert r.status_code == 200 and r.content == b"seed,top_k,top_p"
                for bad in (dict(top_p=0), dict(top_p=1.5), dict(top_k=0), dict(top_k=65), dict(temperature=0),
                            dict(repetition_penalty=-1), dict(seed=-1)):
                    r = await cl.post("/tts", json=dict(character_name="a", text="x", **bad))
                    assert r.status_code == 422, bad
                r = await cl.post("/tts", json=dict(character_name="a", text="x", seed=400))
                assert r.status_code == 400
        finally:
            router.close()
    asyncio.run(run())


# ------------------------------------------------------------------ the oracle helper
def _brute(logits, hist, top_p, rp=1.35):
    """Plain Python float64 loops over steps 1-2: the set of surviving tokens."""
    l = [float(np.float32(v)) for v in logits]
    for t in hist:
        v = np.float32(logits[t])
        l[t] = float(np.float32(v * np.float32(rp)) if v < 0 else np.float32(v / np.float32(rp)))
    mx = max(l)
    e = [math.exp(v - mx) for v in l]
    tot = math.fsum(e)
    order = sorted(range(len(l)), key=lambda i: (-l[i], i))
    keep, s = set(), 0.0
    for r, i in enumerate(order):
        s += e[i] / tot
        if r == 0 or not s > float(np.float32(top_p)):
            keep.add(i)
    return keep


def test_oracle_against_brute_force():
    from tests.philox import sampler_noise
    rng = np.random.default_rng(2024)
    for row in range(20):
        logits = rng.normal(0, 5, size=1025).astype(np.float32)
        if row % 5 == 0:
            logits[rng.choice(1025, 12, replace=False)] = np.float32(4.0)      # ties
        hist = rng.choice(1025, size=int(rng.integers(0, 200)), replace=False)
        top_p = O.pick_top_p([(logits, hist)], (0.3, 0.6, 0.9, 0.99)[row % 4])
        assert O.margin(logits, hist, top_p) >= 1e-6
        keep = O.survivors(O.penalised(logits, hist), top_p).numpy()
        assert set(np.nonzero(keep)[0].tolist()) == _brute(logits, hist, top_p), row
        q = sampler_noise(1025, 1 + row, 0, 77)
        assert O.sample(logits, hist, q, 15, 0.7, top_p=1.0) == O.restate_sample(logits, hist, q, 15, 0.7)
        tok, _ = O.sample(logits, hist, q, 64, 1.0, top_p=top_p)
        assert keep[tok] or np.all(q[keep] < 0)        # a removed token wins only when no survivor has q > 0


def test_gpu_test_inputs_hold_the_margin():
    """The inputs of tests/test_top_p_gpu.py: margin >= 1e-4 on every row (checked here too, so
    a change to them fails without a GPU)."""
    import tests.test_top_p_gpu as T
    cases = []
    for target in (0.5, 0.9, 0.99):
        for top_k, temp in ((15, 0.7), (15, 1.0), (64, 0.7), (64, 1.0)):
            lg, h = T.random_rows(int(target * 100) * 1000 + top_k * 10 + int(temp * 10))
            cases.append((lg, h, O.pick_top_p(list(zip(lg, h)), target)))
    lg, h = T.plateau_rows()
    cases.append((lg, h, O.pick_top_p(list(zip(lg, h)), 0.6)))
    lg, h, _ = T.tie_rows()
    cases.append((lg[:1], h[:1], T.tie_top_p(lg, h)))
    lg, h, _ = T.few_rows()
    cases.append((lg, h, O.pick_top_p(list(zip(lg, h)), 0.75)))
    for lg, h, top_p in cases:
        for b in range(len(h)):
            assert O.margin(lg[b], h[b], top_p) >= O.MARGIN
