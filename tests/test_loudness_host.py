"""CPU: the loudness stage's host side -- the float64 oracle and gsv_loudness_coeffs against the
table of ITU-R BS.1770-4, the oracle's own figures for a full-scale sine and the four test
signals, the gsv_loudness layout, and `loudness` / `peak` carried from api.tts and the server's
/tts payload down to the vocoder item, over a stub engine / worker."""
import asyncio
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import loudness_oracle as O
from tests.test_sample_rate_host import _StubEngine, _stub_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def test_coefficients_match_the_standards_table_at_48000():
    from genie_tts_amd.engine import lib, loudness_coeffs
    want = np.array(TABLE_48K)
    assert np.abs(O.coeffs10(48000) - want).max() <= 1e-12
    assert np.abs(loudness_coeffs(48000) - want).max() <= 1e-12
    c32 = loudness_coeffs(32000)
    assert np.abs(c32 - O.coeffs10(32000)).max() <= 1e-14
    assert np.abs(c32[:5] - [1.5111779, -2.46488941, 1.04163327, -1.5390451, 0.62696686]).max() < 5e-8
    assert np.abs(c32[8:] - [-1.98508967, 0.98514532]).max() < 5e-8
    out = (ctypes.c_double * 10)()
    assert lib().gsv_loudness_coeffs(0, out) == -1 and lib().gsv_loudness_coeffs(-5, out) == -1


def test_full_scale_sine_reads_minus_3_01():
    """A 0 dBFS 997 Hz sine measures -3.01 LKFS (the standard's calibration point)."""
    got = {}
    for fs in (48000, 32000):
        t = np.arange(3 * fs) / fs
        got[fs] = O.loudness(np.sin(2 * np.pi * 997 * t), fs)
    print(f"997 Hz sine: {got[48000]:.4f} at 48 kHz, {got[32000]:.4f} at 32 kHz")
    assert abs(got[48000] + 3.01) <= 0.01
    assert abs(got[32000] - got[48000]) <= 0.1


def test_oracle_figures_of_the_four_signals():
    sig = O.signals()
    assert {k: v.size for k, v in sig.items()} == dict(steady=32000, speech=96000, hum=96000, long=131233)
    m = {k: O.measure(v) for k, v in sig.items()}
    for name, want in (("steady", -12.2125), ("speech", -15.6308), ("hum", -38.7888), ("long", -10.0390)):
        print(f"{name}: {m[name]['loudness']:.4f} LUFS, {m[name]['blocks']} blocks, "
              f"{m[name]['past_abs']} past the absolute gate, {m[name]['blocks_kept']} kept")
        assert abs(m[name]["loudness"] - want) <= 0.005, name
        assert all(v.dtype == np.float32 for v in sig.values())
    assert (m["speech"]["blocks"], m["speech"]["past_abs"], m["speech"]["blocks_kept"]) == (27, 25, 21)
    assert (m["long"]["blocks"], m["long"]["blocks_kept"]) == (38, 31)
    margins = {k: O.gate_margin(v) for k, v in sig.items()}
    assert min(margins.values()) >= 0.5 and abs(margins["long"] - 0.59) < 0.01   # the GPU test relies on it


def test_oracle_rules_the_standard_leaves_open():
    x = O.signals()["steady"]
    assert O.measure(np.zeros(0))["loudness"] == -math.inf and O.measure(np.zeros(0))["blocks_kept"] == 0
    assert O.measure(np.zeros(16000))["blocks_kept"] == 0 and O.loudness(np.zeros(16000)) == -math.inf
    short = O.measure(x[:5000])                                       # one ungated block over all n samples
    y = O.kweight(x[:5000])
    assert short["blocks"] == 1 and short["blocks_kept"] == 1
    assert short["loudness"] == -0.691 + 10 * math.log10((y ** 2).sum() / 5000)
    assert O.measure(x[:12800 + 3199])["loudness"] == O.measure(x[:12800])["loudness"]   # the tail is not measured
    assert O.hops(x).shape == (10,) and O.hops(x[:3199]).shape == (0,)
    imp = np.zeros(16000)
    imp[3199] = 1.0
    assert abs(O.hops(imp)[1] - 0.0832) < 1e-4                        # carried state alone
    assert O.gain(-12.0, 0.3, -16.0) == 10 ** (-4 / 20)
    assert O.gain(-12.0, 0.3, -5.0, 0.5) == 0.5 / 0.3                 # the ceiling
    assert O.gain(-12.0, 0.3, -5.0) == 10 ** (7 / 20) < O.DEFAULT_PEAK / 0.3
    assert O.gain(-math.inf, 0.0, -16.0) == 1.0 and O.gain(-80.0, 1e-4, -16.0, blocks_kept=0) == 1.0
    assert O.gain(-20.0, 0.0, -16.0) == 10 ** (4 / 20)                # peak 0: the first term


def test_loudness_struct_matches_the_c_header(tmp_path):
    from genie_tts_amd.engine import Loudness
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    names = [n for n, _ in Loudness._fields_]
    assert names == ["target", "peak", "stats"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "genie_engine.h"\n'
                   'int main(int argc, char** argv) {\n'
                   '    printf("%zu", sizeof(gsv_loudness));\n' +
                   "".join(f'    printf(" %zu", offsetof(gsv_loudness, {n}));\n' for n in names) +
                   '    printf("\\n");\n'
                   '    gsv_loudness l;\n    memset(&l, 0, sizeof l);\n'
                   '    FILE* f = fopen(argv[1], "rb");\n    if (!f || fread(&l, sizeof l, 1, f) != 1) return 1;\n'
                   '    printf("%g %g %llu\\n", (double)l.target, (double)l.peak, (unsigned long long)(size_t)l.stats);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    blob = tmp_path / "l.bin"
    blob.write_bytes(bytes(Loudness(-16.5, 0.75, 0x1234567890)))
    lines = subprocess.run([str(exe), str(blob)], check=True, capture_output=True, text=True).stdout.splitlines()
    size, *offs = map(int, lines[0].split())
    assert ctypes.sizeof(Loudness) == size == 16
    assert [getattr(Loudness, n).offset for n in names] == offs == [0, 4, 8]
    assert lines[1].split() == ["-16.5", "0.75", str(0x1234567890)]
    zero = Loudness()                                               # zero: off for this item
    assert (zero.target, zero.peak, zero.stats) == (0.0, 0.0, None)


def test_check_loudness():
    from genie_tts_amd.engine import check_loudness
    assert check_loudness() == {} and check_loudness(None, 0.5) == {}
    assert check_loudness(-16) == {"loudness": -16.0} and check_loudness(-23.0, 1) == {"loudness": -23.0, "peak": 1.0}
    assert check_loudness(-50, 1e-3) == {"loudness": -50.0, "peak": 1e-3} and check_loudness(-5) == {"loudness": -5.0}
    assert check_loudness(np.float32(-16)) == {"loudness": -16.0}
    for bad in (0, 0.0, -4.99, -50.01, 3, float("nan"), float("inf"), -float("inf"), "-16", True, [-16]):
        with pytest.raises(ValueError):
            check_loudness(bad)
    for bad in (0, 0.0, -0.5, 1.0001, float("nan"), "0.5", False):
        with pytest.raises(ValueError):
            check_loudness(-16, bad)
        with pytest.raises(ValueError):
            check_loudness(None, bad)                                 # a bad ceiling is bad with or without a target


def test_exported_symbols_and_header_agree():
    from genie_tts_amd.engine import EXPORTED, lib
    hdr = open(os.path.join(ROOT, "include", "genie_engine.h")).read()
    for name in ("gsv_loudness_coeffs", "gsv_vits_decode_item_norm", "gsv_vits_decode_batch_norm",
                 "gsv_vits_decode_batch_async_norm", "gsv_vits_decode_async_norm", "gsv_audio_loudness",
                 "gsv_audio_normalize", "gsv_debug_loudness_hops"):
        assert name in EXPORTED and f"int {name}(" in hdr and getattr(lib(), name)


# ------------------------------------------------------------------ api over a stub engine
def _fmt(call):
    """The output-format and loudness keys of a recorded vocoder call."""
    return {k: call[k] for k in ("sample_rate", "pcm16", "loudness", "peak") if k in call}


def test_api_tts_loudness_reaches_the_vocoder_item(monkeypatch, tmp_path):
    eng = _StubEngine(G=11)
    api = _stub_model(monkeypatch, eng)
    txt = np.array([3, 5, 7], np.int64)
    out = api.tts("sr-c", txt, loudness=-16)
    assert [_fmt(c) for c in eng.calls] == [dict(loudness=-16.0)]             # alone: float32 at 32 kHz, normalised
    assert out.dtype == np.float32 and out.shape == (1280 * 11,)
    eng.calls.clear()
    api.tts("sr-c", txt, loudness=-23.0, peak=0.5, sample_rate=16000)
    assert [_fmt(c) for c in eng.calls] == [dict(loudness=-23.0, peak=0.5, sample_rate=16000)]
    eng.calls.clear()
    api.tts("sr-c", txt)
    assert [_fmt(c) for c in eng.calls] == [{}]                             # today's call, unchanged
    api.tts("sr-c", txt, peak=0.5)
    assert _fmt(eng.calls[-1]) == {}                           # a ceiling without a target: nothing to do
    n = len(eng.calls)
    for bad in (dict(loudness=-4), dict(loudness=0), dict(loudness="x"), dict(loudness=-16, peak=0),
                dict(loudness=-16, peak=1.5), dict(peak=-1)):
        with pytest.raises(ValueError):
            api.tts("sr-c", txt, **bad)
    assert len(eng.calls) == n                                        # rejected before any synthesis

    async def go(**kw):
        return [c async for c in api.tts_async("sr-c", txt, **kw)]
    chunks = asyncio.run(go(loudness=-16, sample_rate=48000))
    assert [len(c) for c in chunks] == [2 * 1920 * 11]
    assert _fmt(eng.calls[-1]) == dict(loudness=-16.0, sample_rate=48000, pcm16=True)
    chunks = asyncio.run(go(loudness=-16, peak=0.9))
    assert [len(c) for c in chunks] == [2 * 1280 * 11]                # float32 from the GPU, PCM on the host
    assert _fmt(eng.calls[-1]) == dict(loudness=-16.0, peak=0.9)
    with pytest.raises(ValueError):
        asyncio.run(go(loudness=-60))


def test_tts_batch_vocoder_takes_one_value_or_one_per_item(monkeypatch):
    from types import SimpleNamespace
    from genie_tts_amd.inference import tts_client
    seen = []

    class V:
        engine = None
        noise_scale = 0.5

        def run(self, names, feed):
            seen.append({k: feed[k] for k in ("loudness", "peak", "sample_rate", "pcm16") if k in feed})
            return [np.zeros(4, np.float32)]
    m = SimpleNamespace(ENGINE=object(), VITS=V(), PROMPT_ENCODER=None)
    ref = SimpleNamespace(audio_32k=np.zeros((1, 64), np.float32))
    items = [(np.zeros((1, 3), np.int64), None)] * 3
    toks = [np.arange(5)] * 3
    tts_client.tts_batch_vocoder(items, toks, ref, m, loudness=-16)
    assert seen == [dict(loudness=-16.0)] * 3
    seen.clear()
    tts_client.tts_batch_vocoder(items, toks, ref, m, loudness=[-16, None, -23], peak=[None, 0.5, 0.25],
                                 sample_rate=[None, 8000, 48000], pcm16=[False, True, True])
    assert seen == [dict(loudness=-16.0), dict(sample_rate=8000, pcm16=True),
                    dict(loudness=-23.0, peak=0.25, sample_rate=48000, pcm16=True)]
    seen.clear()
    tts_client.tts_batch_vocoder(items, toks, ref, m)
    assert seen == [{}] * 3
    for bad in (dict(loudness=[-16, -16]), dict(loudness=-16, peak=[0.5]), dict(loudness=[-16, -4, -16]),
                dict(loudness=-3)):
        with pytest.raises(ValueError):
            tts_client.tts_batch_vocoder(items, toks, ref, m, **bad)
    assert seen == [{}] * 3


# ------------------------------------------------------------------ the server
def _loud_worker(index, conn, cfg):
    """Replies like _worker_main: one chunk whose four samples hold -loudness, 100 * peak (0: none)."""
    conn.send(dict(kind="ready", id=-1, index=index))
    while True:
        msg = conn.recv()
        if msg is None:
            return
        if msg["cmd"] == "tts":
            v = [int(round(-(msg.get("loudness") or 0))), int(round(100 * (msg.get("peak") or 0)))] * 2
            conn.send(dict(kind="chunk", id=msg["id"], data=np.array(v, np.int16).tobytes()))
            conn.send(dict(kind="end", id=msg["id"]))
        else:
            conn.send(dict(kind="ok", id=msg["id"]))


def test_tts_payload_loudness_validation():
    import httpx
    from genie_tts_amd.server import Router, create_app

    async def run():
        router = Router([0], worker=_loud_worker)
        router.start(asyncio.get_running_loop(), timeout=120)
        tr = httpx.ASGITransport(app=create_app(router))
        try:
            async with httpx.AsyncClient(transport=tr, base_url="http://t") as cl:
                r = await cl.post("/tts", json=dict(character_name="a", text="x"))
                assert r.status_code == 200 and np.frombuffer(r.content, np.int16).tolist() == [0] * 4
                assert "x-loudness" not in r.headers
                r = await cl.post("/tts", json=dict(character_name="a", text="x", loudness=-16))
                assert r.status_code == 200 and np.frombuffer(r.content, np.int16).tolist() == [16, 0] * 2
                assert r.headers["x-loudness"] == "-16" and "x-sample-rate" not in r.headers
                r = await cl.post("/tts", json=dict(character_name="a", text="x", loudness=-23.5, peak=0.5,
                                                    sample_rate=48000))
                assert r.status_code == 200 and np.frombuffer(r.content, np.int16).tolist() == [24, 50] * 2
                assert r.headers["x-loudness"] == "-23.5" and r.headers["x-sample-rate"] == "48000"
                for bad in (dict(loudness=-4), dict(loudness=0), dict(loudness=-51), dict(loudness=-16, peak=0),
                            dict(loudness=-16, peak=1.5), dict(peak=-0.5)):
                    r = await cl.post("/tts", json=dict(character_name="a", text="x", **bad))
                    assert r.status_code == 400 and r.json()["detail"].startswith("loudness:"), bad
                r = await cl.post("/tts", json=dict(character_name="a", text="x", loudness="loud"))
                assert r.status_code == 422
        finally:
            router.close()
    asyncio.run(run())


def test_worker_carries_loudness_into_the_round(monkeypatch):
    """_worker_main's accept(): the request's target and ceiling reach the round's vocoder items per
    item, a bad value fails that request only, and a request without one is today's call."""
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
        T2S_FIRST_STAGE_DECODER = type("D", (), {"sampler": None})()

    seen = []

    def vocoder(items, toks, ref, m, overlapped=False, speed=1.0, **fmt):
        seen.append(fmt)
        return [np.full(1280 * 11, 0.5, np.float32) for _ in items]

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
        parent.send(dict(cmd="tts", id=1, character_name="a", text="かき。", loudness=-16, peak=0.5))
        got = collect(1)
        assert [m["kind"] for m in got] == ["chunk", "end"]
        assert got[0]["data"] == np.full(1280 * 11, 16383, np.int16).tobytes()   # float32 from the vocoder, PCM here
        assert seen == [dict(loudness=[-16.0], peak=[0.5])]
        parent.send(dict(cmd="tts", id=2, character_name="a", text="かき。", loudness=-16, sample_rate=8000))
        collect(2)
        assert seen[-1] == dict(sample_rate=[8000], pcm16=[True], loudness=[-16.0], peak=[None])
        for i, bad in enumerate((dict(loudness=-4), dict(loudness=-16, peak=2), dict(loudness="x")), 3):
            parent.send(dict(cmd="tts", id=i, character_name="a", text="かき。", **bad))
            got = collect(i)
            assert [m["kind"] for m in got] == ["error"] and got[0]["detail"].startswith("loudness:"), bad
        parent.send(dict(cmd="tts", id=9, character_name="a", text="かき。"))      # none: today's call
        assert [m["kind"] for m in collect(9)] == ["chunk", "end"]
        assert seen[-1] == {} and len(seen) == 3
    finally:
        parent.send(None)
        t.join(timeout=30)
        api.set_g2p(None)
