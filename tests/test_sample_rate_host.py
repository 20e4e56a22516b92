"""CPU: the output stage's host side -- the numpy oracle of the resample against
scipy.signal.resample_poly, gsv_audio_samples (the one place the output length is computed), the
gsv_vits_item layout with its three new fields, and `sample_rate` carried from api.tts / the
server's /tts payload down to the vocoder item, over a stub engine / worker."""
import asyncio
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import resample_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = tuple(r for r in O.RATES if r != 32000)


@pytest.mark.parametrize("rate", SIX)
def test_oracle_against_scipy_resample_poly(rate):
    from scipy.signal import resample_poly
    up, down = O.ratio(rate)
    rng = np.random.default_rng(rate)
    for n in (1, 7, 640, 2561):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        want = resample_poly(x.astype(np.float64), up, down)
        got = O.resample(x, rate)
        assert got.shape == want.shape == (O.n_out(n, rate),)
        err = float(np.abs(got - want).max())
        print(f"{rate} Hz n_in {n}: n_out {got.size}, max abs vs scipy {err:.2e}")
        assert err <= 1e-12


def test_oracle_pcm16_rule():
    y = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.6, -1.6, 0.99999, 3.05e-5, -3.05e-5])
    assert O.pcm16(y).tolist() == [0, 16383, -16383, 32767, -32767, 32767, -32768, 32766, 0, 0]
    x = np.random.default_rng(0).uniform(-1, 1, 1000).astype(np.float32)
    from genie_tts_amd import audio as A
    ref = np.frombuffer(A.to_pcm16(x), np.int16).astype(np.int32)   # the reference's rule, its product in float32
    assert np.abs(O.pcm16(x).astype(np.int32) - ref).max() <= 1     # the float64 product truncates one step apart


def test_audio_samples_rule():
    from genie_tts_amd.engine import audio_samples, lib
    assert [O.ratio(r) for r in O.RATES] == [(1, 4), (1, 2), (441, 640), (3, 4), (1, 1), (441, 320), (3, 2)]
    for rate in O.RATES:
        up, down = O.ratio(rate)
        for n in (0, 1, 7, 640, 2561, 102400, 640 * 4096):
            want = -(-n * up // down)
            assert lib().gsv_audio_samples(n, rate) == want == audio_samples(n, rate), (n, rate)
    assert lib().gsv_audio_samples(640, 0) == 640                   # 0 means 32000
    for bad in O.BAD_RATES:
        assert lib().gsv_audio_samples(640, bad) == -1, bad         # GSV_E_ARG
        with pytest.raises(ValueError):
            audio_samples(640, bad)
    assert lib().gsv_audio_samples(-1, 16000) == -1
    for bad in (None, 16000.5, "16000", True):
        with pytest.raises(ValueError):
            audio_samples(640, bad)


def test_vits_item_struct_matches_the_c_header(tmp_path):
    """The three fields follow `speed`; everything before them stays where it was."""
    from genie_tts_amd.engine import VitsItem
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    names = [n for n, _ in VitsItem._fields_]
    assert names[-4:] == ["speed", "out_rate", "out_format", "out"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "genie_engine.h"\n'
                   'int main(int argc, char** argv) {\n'
                   '    printf("%zu", sizeof(gsv_vits_item));\n' +
                   "".join(f'    printf(" %zu", offsetof(gsv_vits_item, {n}));\n' for n in names) +
                   '    printf("\\n");\n'
                   '    gsv_vits_item it;\n    memset(&it, 0, sizeof it);\n'
                   '    FILE* f = fopen(argv[1], "rb");\n    if (!f || fread(&it, sizeof it, 1, f) != 1) return 1;\n'
                   '    printf("%d %d %llu %g %d\\n", (int)it.out_rate, (int)it.out_format,\n'
                   '           (unsigned long long)(size_t)it.out, (double)it.speed, (int)it.n_sem);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    it = VitsItem()                                                 # filled through ctypes, read back in C
    it.n_sem, it.speed, it.out_rate, it.out_format, it.out = 12, 1.25, 44100, 1, 0x1234567890
    blob = tmp_path / "item.bin"
    blob.write_bytes(bytes(it))
    lines = subprocess.run([str(exe), str(blob)], check=True, capture_output=True, text=True).stdout.splitlines()
    size, *offs = map(int, lines[0].split())
    assert ctypes.sizeof(VitsItem) == size
    assert [getattr(VitsItem, n).offset for n in names] == offs
    assert lines[1].split() == ["44100", "1", str(0x1234567890), "1.25", "12"]
    zero = VitsItem()                                               # a zero tail: "as before"
    assert (zero.out_rate, zero.out_format, zero.out) == (0, 0, None)


# ------------------------------------------------------------------ api over a stub engine
class _StubEngine:
    """Stands in for Engine under the real sessions and GENIE driver: fixed tokens, and a
    vocoder that records its call and returns zeros of the length and dtype asked for."""
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
        from genie_tts_amd.engine import audio_samples
        self.calls.append(dict(kw, speed=speed))
        n = 640 * self.vits_frames(np.asarray(sem).size, speed)
        if kw.get("sample_rate") is not None:
            n = audio_samples(n, kw["sample_rate"])
        return torch.zeros(n, dtype=torch.int16 if kw.get("pcm16") else torch.float32)


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
    monkeypatch.setitem(api._reference_audios, "sr-c", ref)
    return api


def test_api_tts_sample_rate_reaches_the_vocoder_item(monkeypatch, tmp_path):
    import wave
    eng = _StubEngine(G=11)
    api = _stub_model(monkeypatch, eng)
    txt = np.array([3, 5, 7], np.int64)
    wav = tmp_path / "o.wav"
    out = api.tts("sr-c", txt, sample_rate=16000, save_path=str(wav))
    assert [c.get("sample_rate") for c in eng.calls] == [16000] and not eng.calls[0].get("pcm16")
    assert out.dtype == np.float32 and out.shape == (640 * 11,)     # 1280 * 11 samples at half the rate
    with wave.open(str(wav)) as f:
        assert f.getframerate() == 16000 and f.getnframes() == 640 * 11
    eng.calls.clear()
    assert api.tts("sr-c", txt, save_path=str(wav)).shape == (1280 * 11,)
    assert "sample_rate" not in eng.calls[0] and "pcm16" not in eng.calls[0]   # today's call, unchanged
    with wave.open(str(wav)) as f:
        assert f.getframerate() == 32000
    for bad in (12345, 11025, 0, 16000.5, "16000"):
        with pytest.raises(ValueError):
            api.tts("sr-c", txt, sample_rate=bad)
    assert len(eng.calls) == 1                                      # rejected before any synthesis

    async def go(**kw):
        return [c async for c in api.tts_async("sr-c", txt, **kw)]
    chunks = asyncio.run(go(sample_rate=48000, save_path=str(wav)))
    assert [len(c) for c in chunks] == [2 * 1920 * 11]
    assert eng.calls[-1]["sample_rate"] == 48000 and eng.calls[-1]["pcm16"] is True
    with wave.open(str(wav)) as f:
        assert f.getframerate() == 48000 and f.getnframes() == 1920 * 11
    chunks = asyncio.run(go())
    assert [len(c) for c in chunks] == [2 * 1280 * 11] and "sample_rate" not in eng.calls[-1]
    with pytest.raises(ValueError):
        asyncio.run(go(sample_rate=12345))


# ------------------------------------------------------------------ the server
def _rate_worker(index, conn, cfg):
    """Replies like _worker_main: one chunk whose samples all hold sample_rate / 100 (0: none)."""
    conn.send(dict(kind="ready", id=-1, index=index))
    while True:
        msg = conn.recv()
        if msg is None:
            return
        if msg["cmd"] == "tts":
            conn.send(dict(kind="chunk", id=msg["id"],
                           data=np.full(4, (msg.get("sample_rate") or 0) // 100, np.int16).tobytes()))
            conn.send(dict(kind="end", id=msg["id"]))
        else:
            conn.send(dict(kind="ok", id=msg["id"]))


def test_tts_payload_sample_rate_validation():
    import httpx
    from genie_tts_amd.server import Router, create_app

    async def run():
        router = Router([0], worker=_rate_worker)
        router.start(asyncio.get_running_loop(), timeout=120)
        tr = httpx.ASGITransport(app=create_app(router))
        try:
            async with httpx.AsyncClient(transport=tr, base_url="http://t") as cl:
                r = await cl.post("/tts", json=dict(character_name="a", text="x"))
                assert r.status_code == 200 and np.frombuffer(r.content, np.int16).tolist() == [0] * 4
                assert "x-sample-rate" not in r.headers
                for rate in O.RATES:
                    r = await cl.post("/tts", json=dict(character_name="a", text="x", sample_rate=rate))
                    assert r.status_code == 200 and np.frombuffer(r.content, np.int16).tolist() == [rate // 100] * 4
                    assert r.headers["x-sample-rate"] == str(rate)
                for bad in (12345, 11025, 0, -8000, "fast", 16000.5):
                    r = await cl.post("/tts", json=dict(character_name="a", text="x", sample_rate=bad))
                    assert r.status_code == 422, bad
        finally:
            router.close()
    asyncio.run(run())


def test_worker_carries_sample_rate_into_the_round(monkeypatch, tmp_path):
    """_worker_main's accept(): the request's rate reaches the round's vocoder items (per item,
    with pcm16), the chunk is the int16 samples the vocoder returned, save_path's header has the
    rate, a bad rate fails that request only, and a request without one is today's call."""
    import multiprocessing as mp
    import threading
    import wave
    from genie_tts_amd import api
    from genie_tts_amd.engine import audio_samples
    from genie_tts_amd.inference import tts_client
    from genie_tts_amd.model_manager import model_manager
    from genie_tts_amd.server import _worker_main

    class M:
        LANGUAGE = "Japanese"
        ENGINE = None
        VITS = None
        T2S_FIRST_STAGE_DECODER = type("D", (), {"sampler": None})()

    seen = []

    def vocoder(items, toks, ref, m, overlapped=False, speed=1.0, **fmt):
        seen.append(fmt)
        if not fmt:
            return [np.full(1280 * 11, 0.5, np.float32) for _ in items]
        return [np.full(audio_samples(1280 * 11, r), 7, np.int16) if r is not None else np.zeros(1280 * 11, np.float32)
                for r in fmt["sample_rate"]]

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
        wav = str(tmp_path / "s.wav")
        parent.send(dict(cmd="tts", id=1, character_name="a", text="かき。", sample_rate=44100, save_path=wav))
        got = collect(1)
        assert [m["kind"] for m in got] == ["chunk", "end"]
        n = audio_samples(1280 * 11, 44100)
        assert got[0]["data"] == np.full(n, 7, np.int16).tobytes()  # the vocoder's int16, untouched
        assert seen == [dict(sample_rate=[44100], pcm16=[True])]
        with wave.open(wav) as f:
            assert f.getframerate() == 44100 and f.getnframes() == n
        parent.send(dict(cmd="tts", id=2, character_name="a", text="かき。", sample_rate=12345))
        got = collect(2)
        assert [m["kind"] for m in got] == ["error"] and got[0]["detail"].startswith("sample_rate:")
        parent.send(dict(cmd="tts", id=3, character_name="a", text="かき。"))     # no rate: today's call
        got = collect(3)
        assert [m["kind"] for m in got] == ["chunk", "end"]
        assert got[0]["data"] == np.full(1280 * 11, 16383, np.int16).tobytes()   # host to_pcm16 of 0.5
        assert seen[-1] == {} and len(seen) == 2
    finally:
        parent.send(None)
        t.join(timeout=30)
        api.set_g2p(None)
