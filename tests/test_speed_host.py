"""CPU: the speech-rate control's host side -- gsv_vits_frames (the one place T' is
computed), the numpy restatement of the resample against torch's F.interpolate within the
derived bound (it is the bit-exact oracle of the GPU tests), and `speed` carried from
api.tts / the server's /tts payload down to the vocoder item, over a stub engine / worker."""
import asyncio
import ctypes
import math

import numpy as np
import pytest

from tests.speed_oracle import interp_bound, interp_linear_np


def _frames(n_sem, speed):
    from genie_tts_amd.engine import lib
    return lib().gsv_vits_frames(n_sem, ctypes.c_float(speed))


def test_vits_frames_rule():
    for n in (1, 8, 11, 80, 1000):
        assert _frames(n, 0.0) == 2 * n and _frames(n, 1.0) == 2 * n
    # T' = (int)((double)T / (double)(float32 speed)) + 1, values worked out by hand:
    # 22 / f32(1.1) = 19.99999957 -> 20 (the double 1.1 would give int(20.000000000000004) + 1 = 21)
    table = [(11, 1.1, 20), (8, 0.5, 33), (8, 0.8, 20), (8, 1.25, 13), (8, 2.0, 9), (80, 0.9, 178), (80, 1.1, 146),
             (80, 0.8, 200), (80, 1.25, 129), (1, 4.0, 1), (1, 0.25, 9), (5, 3.0, 4), (1024, 0.5, 4097)]
    for n, sp, want in table:
        assert _frames(n, sp) == want, (n, sp)
        assert want == int((2 * n) / float(np.float32(sp))) + 1     # the rule, float32 widened to double
    assert int(22 / 1.1) + 1 == 21                                  # ... which a Python double misses
    for bad in (math.nan, math.inf, -1.0, 0.2, 4.5):
        assert _frames(8, bad) == -1, bad                           # GSV_E_ARG


def test_engine_vits_frames_raises():
    from genie_tts_amd.engine import Engine, vits_frames
    assert Engine.vits_frames(11, 1.1) == 20 and vits_frames(11) == 22
    for bad in (math.nan, 0.2, 4.5, "fast"):
        with pytest.raises(ValueError):
            vits_frames(8, bad)


@pytest.mark.parametrize("T", [2, 3, 16, 17, 160])
def test_numpy_resample_against_torch_interpolate(T):
    import torch
    import torch.nn.functional as F
    y = np.random.default_rng(T).standard_normal((192, T)).astype(np.float32)
    for sp in (0.5, 0.8, 1.25, 2.0):
        To = _frames(T // 2, sp) if T % 2 == 0 else int(T / float(np.float32(sp))) + 1
        got = interp_linear_np(y, To)
        assert got.dtype == np.float32 and got.shape == (192, To)
        ref = F.interpolate(torch.from_numpy(y)[None], size=To, mode="linear")[0].numpy()
        err = np.abs(got.astype(np.float64) - ref)
        bound = interp_bound(y, To)
        print(f"T {T} speed {sp}: T' {To}, max err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), (T, sp, float((err / bound).max()))
    assert np.array_equal(interp_linear_np(y, T), y)                # T' = T: the identity


# ------------------------------------------------------------------ api over a stub engine
class _StubEngine:
    """Stands in for Engine under the real sessions and GENIE driver: fixed tokens, and a
    vocoder that records its call and returns 640 T' zeros."""
    vocoder_cus = 0

    def __init__(self, G=11):
        self.G = G
        self.calls = []

    @staticmethod
    def vits_frames(n_sem, speed=1.0):
        from genie_tts_amd.engine import vits_frames
        return vits_frames(n_sem, speed)

    def t2s_generate(self, utts, sampler):
        return [np.arange(self.G, dtype=np.int64) for _ in utts]

    def ref_encode(self, audio):
        return np.zeros(512, np.float32)

    def vits_decode(self, text_seq, sem, speed=1.0, **kw):
        import torch
        self.calls.append(dict(kw, speed=speed, G=int(np.asarray(sem).size)))
        return torch.zeros(640 * self.vits_frames(np.asarray(sem).size, speed))


def _stub_model(monkeypatch, eng):
    from types import SimpleNamespace
    from genie_tts_amd import api
    from genie_tts_amd.inference import ReferenceAudio
    from genie_tts_amd.sessions import (EncoderSession, FirstStageDecoderSession, StageDecoderSession, VitsSession,
                                        _T2SState)
    st = _T2SState()
    m = SimpleNamespace(T2S_ENCODER=EncoderSession(eng), T2S_FIRST_STAGE_DECODER=FirstStageDecoderSession(eng, None, st),
                        T2S_STAGE_DECODER=StageDecoderSession(eng, None, st), VITS=VitsSession(eng, "v2", noise="zero"),
                        PROMPT_ENCODER=None, LANGUAGE="Japanese", ENGINE=eng)
    monkeypatch.setattr(api.model_manager, "get", lambda name: m)
    ref = ReferenceAudio(phonemes_seq=np.zeros((1, 4), np.int64), text_bert=np.zeros((4, 1024), np.float32),
                         audio_32k=np.zeros((1, 4096), np.float32), ssl_content=np.zeros((1, 768, 8), np.float32))
    monkeypatch.setitem(api._reference_audios, "sp-c", ref)
    return api


def test_api_tts_speed_reaches_the_vocoder_item(monkeypatch, tmp_path):
    eng = _StubEngine(G=11)
    api = _stub_model(monkeypatch, eng)
    txt = np.array([3, 5, 7], np.int64)
    wav = tmp_path / "o.wav"
    out = api.tts("sp-c", txt, speed=1.1, save_path=str(wav))
    assert [c["speed"] for c in eng.calls] == [pytest.approx(1.1)]
    assert out.shape == (640 * 20,)                                 # T' = 20 at n_sem 11 (not 21)
    import wave
    with wave.open(str(wav)) as f:
        assert f.getnframes() == 640 * 20                           # save_path holds the same audio
    eng.calls.clear()
    assert api.tts("sp-c", txt).shape == (1280 * 11,)
    assert api.tts("sp-c", txt, speed=1.0).shape == (1280 * 11,)
    assert [c["speed"] for c in eng.calls] == [1.0, 1.0]
    for bad in (0.2, 4.5, math.nan):
        with pytest.raises(ValueError):
            api.tts("sp-c", txt, speed=bad)
    assert len(eng.calls) == 2                                      # rejected before any synthesis

    async def go():
        return [c async for c in api.tts_async("sp-c", txt, speed=2.0)]
    chunks = asyncio.run(go())
    assert [len(c) for c in chunks] == [2 * 640 * 12] and eng.calls[-1]["speed"] == 2.0


def test_vits_session_speed_feed_and_eps_fn():
    from genie_tts_amd.sessions import VitsSession
    eng = _StubEngine()
    seen = []

    def eps_fn(G, frames=None):
        seen.append((G, frames))
        return np.zeros((192, frames or 2 * G), np.float32)
    s = VitsSession(eng, "v2", eps_fn=eps_fn)
    feed = dict(text_seq=np.zeros((1, 3), np.int64), pred_semantic=np.zeros((1, 1, 8), np.int64),
                ref_audio=np.zeros((1, 4096), np.float32))
    assert s.run(None, feed)[0].shape == (1280 * 8,)
    assert s.run(None, dict(feed, speed=np.float32(0.8)))[0].shape == (640 * 20,)
    assert seen == [(8, None), (8, 20)] and eng.calls[-1]["eps"].shape == (192, 20)
    with pytest.raises(ValueError):
        s.run(None, dict(feed, speed=5.0))


# ------------------------------------------------------------------ the server
def _speed_worker(index, conn, cfg):
    """Replies like _worker_main: one chunk whose samples all hold round(100 * speed)."""
    conn.send(dict(kind="ready", id=-1, index=index))
    while True:
        msg = conn.recv()
        if msg is None:
            return
        if msg["cmd"] == "tts":
            conn.send(dict(kind="chunk", id=msg["id"],
                           data=np.full(4, round(100 * msg["speed"]), np.int16).tobytes()))
            conn.send(dict(kind="end", id=msg["id"]))
        else:
            conn.send(dict(kind="ok", id=msg["id"]))


def test_tts_payload_speed_validation():
    import httpx
    from genie_tts_amd.server import Router, create_app

    async def run():
        router = Router([0], worker=_speed_worker)
        router.start(asyncio.get_running_loop(), timeout=120)
        tr = httpx.ASGITransport(app=create_app(router))
        try:
            async with httpx.AsyncClient(transport=tr, base_url="http://t") as cl:
                r = await cl.post("/tts", json=dict(character_name="a", text="x"))
                assert r.status_code == 200 and np.frombuffer(r.content, np.int16).tolist() == [100] * 4
                r = await cl.post("/tts", json=dict(character_name="a", text="x", speed=1.25))
                assert r.status_code == 200 and np.frombuffer(r.content, np.int16).tolist() == [125] * 4
                for bad in (0.2, 4.5, -1, "fast"):
                    r = await cl.post("/tts", json=dict(character_name="a", text="x", speed=bad))
                    assert r.status_code == 422, bad
        finally:
            router.close()
    asyncio.run(run())


def test_worker_carries_speed_into_the_round(monkeypatch):
    """_worker_main's accept(): the request's speed reaches the round's vocoder items (per
    item), the PCM chunk has 640 T' samples, and a bad speed fails that request only."""
    import multiprocessing as mp
    import threading
    from genie_tts_amd import api
    from genie_tts_amd.engine import vits_frames
    from genie_tts_amd.inference import tts_client
    from genie_tts_amd.model_manager import model_manager
    from genie_tts_amd.server import _worker_main

    class M:
        LANGUAGE = "Japanese"
        ENGINE = None
        VITS = None
        T2S_FIRST_STAGE_DECODER = type("D", (), {"sampler": None})()

    seen = []

    def vocoder(items, toks, ref, m, overlapped=False, speed=1.0):
        seen.append(speed)
        sp = [speed] * len(items) if np.ndim(speed) == 0 else speed
        return [np.zeros(640 * vits_frames(11, v), np.float32) for v in sp]

    monkeypatch.setattr(model_manager, "get", lambda name: M())
    monkeypatch.setitem(api._reference_audios, "a", object())
    monkeypatch.setattr(tts_client, "tts_batch_t2s", lambda items, ref, m, sp: [None] * len(items))
    monkeypatch.setattr(tts_client, "tts_batch_vocoder", vocoder)
    parent, child = mp.Pipe()
    t = threading.Thread(target=_worker_main, args=(0, child, {"g2p": "genie_tts_amd.stubs:toy_g2p"}), daemon=True)
    t.start()

    def collect(rid):
        out = []
        while True:
            assert parent.poll(60), "worker did not answer"
            m = parent.recv()
            if m["id"] == rid:
                out.append(m)
                if m["kind"] in ("end", "error"):
                    return out
    try:
        assert parent.poll(60) and parent.recv()["kind"] == "ready"
        parent.send(dict(cmd="tts", id=1, character_name="a", text="かき。", speed=1.1))
        got = collect(1)
        assert [m["kind"] for m in got] == ["chunk", "end"] and len(got[0]["data"]) == 2 * 640 * 20
        assert seen == [[pytest.approx(1.1)]]
        parent.send(dict(cmd="tts", id=2, character_name="a", text="かき。", speed=9.0))
        got = collect(2)
        assert [m["kind"] for m in got] == ["error"] and got[0]["detail"].startswith("speed:")
        parent.send(dict(cmd="tts", id=3, character_name="a", text="かき。"))     # no speed: today's call
        got = collect(3)
        assert [m["kind"] for m in got] == ["chunk", "end"] and len(got[0]["data"]) == 2 * 1280 * 11
        assert seen[-1] == 1.0 and len(seen) == 2
    finally:
        parent.send(None)
        t.join(timeout=30)
        api.set_g2p(None)
