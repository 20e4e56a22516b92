"""GPU: the output stage (sample rate and 16-bit PCM; include/genie_engine.h, gsv_audio_convert)
-- the kernel alone against the float64 oracle (tests/resample_oracle.py, pinned to
scipy.signal.resample_poly by tests/test_sample_rate_host.py), behind every vocoder entry point,
and from api.tts / the server's /tts down.

Bounds.  Float output: max abs <= 1.2e-5 = (N + 1) * 2^-24 * sum|h| * max|x| with N <= 81 taps, the
per-phase sum of |h| <= 2.25 and |x| <= 1 (the same float32 chain on the CPU measured 3.3e-7; the
GPU's figure is in DESIGN §4.3c).  int16 output: within 1 of the oracle
everywhere, and equal wherever the oracle's y * 32767 lies further than 0.4 from an integer
(1.2e-5 * 32767 = 0.39).  Behind the vocoder the stage's output equals gsv_audio_convert of the
same call's 32 kHz audio bit for bit: one float32 chain per output, whatever the entry point.
"""
import asyncio
import ctypes
import wave

import numpy as np
import pytest

from genie_tts_amd import synth
from tests import resample_oracle as O
from tests.common import character

pytestmark = pytest.mark.gpu

BOUND = 1.2e-5
N_TILES = 3301          # n_in whose outputs span >= 3 tiles of 256 and a remainder at every rate (8 kHz: 826)
SIZES = (1, 7, 639, 640, 2561, N_TILES)
_engines = {}


def _engine(ver):
    from genie_tts_amd.engine import Engine
    if ver not in _engines:
        w = character(ver)
        _engines[ver] = Engine({k: w[k] for k in ("t2s_encoder", "t2s", "vits", "prompt_encoder") if k in w}, ver)
    return _engines[ver]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture(scope="module", params=["v2", "v2ProPlus"])
def setup(request):
    return request.param, _engine(request.param)


def _x(n, rate):
    return np.random.default_rng(1000 * n + rate).uniform(-1, 1, n).astype(np.float32)


def _convert_guarded(e, x, rate, fmt):
    """gsv_audio_convert into a buffer pre-filled with a sentinel, one guard element past n_out."""
    import torch
    from genie_tts_amd.engine import _check, _stream, lib
    n_out = lib().gsv_audio_samples(x.size, rate)
    assert n_out == O.n_out(x.size, rate or 32000)
    xd = torch.from_numpy(x).to(e.dev)
    if fmt == 0:
        out = torch.full((n_out + 1,), float("nan"), dtype=torch.float32, device=e.dev)
    else:
        out = torch.full((n_out + 1,), -12345, dtype=torch.int16, device=e.dev)
    _check(lib().gsv_audio_convert(e.h, ctypes.c_void_p(xd.data_ptr()), x.size, rate, fmt,
                                   ctypes.c_void_p(out.data_ptr()), _stream()), "gsv_audio_convert")
    got = out.cpu().numpy()
    assert np.isnan(got[-1]) if fmt == 0 else got[-1] == -12345, "the guard element was written"
    return got[:-1]


@pytest.mark.parametrize("rate", [r for r in O.RATES if r != 32000])
def test_kernel_alone_against_the_oracle(rate):
    e = _engine("v2")
    if rate == 48000:   # saturation is exercised: the resampled signal overshoots +-1
        y = O.resample(_x(N_TILES, rate), rate)
        assert y.max() > 1.0 and y.min() < -1.0
    worst = 0.0
    for n in SIZES:
        x = _x(n, rate)
        want = O.resample(x, rate)
        got = _convert_guarded(e, x, rate, 0)
        assert got.shape == want.shape and not np.isnan(got).any(), (rate, n)
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst = max(worst, err)
        print(f"{rate} Hz n_in {n}: n_out {got.size}, max abs err {err:.2e}")
        assert err <= BOUND, (rate, n, err)
        pcm = _convert_guarded(e, x, rate, 1).astype(np.int64)
        wpcm = O.pcm16(want).astype(np.int64)
        assert np.abs(pcm - wpcm).max() <= 1, (rate, n)
        v = np.clip(want * 32767.0, -32768.0, 32767.0)
        sure = np.abs(v - np.round(v)) > 0.4
        assert np.array_equal(pcm[sure], wpcm[sure]), (rate, n)
        assert np.array_equal(e.audio_convert(x, rate).cpu().numpy(), got)                 # the Python binding
        assert np.array_equal(e.audio_convert(x, rate, pcm16=True).cpu().numpy(), pcm)
    print(f"{rate} Hz: worst max abs err {worst:.2e} (bound {BOUND:.1e})")


def test_kernel_alone_at_32000_is_a_copy():
    from genie_tts_amd import audio as A
    e = _engine("v2")
    for n in SIZES:
        x = _x(n, 32000)
        assert np.array_equal(_convert_guarded(e, x, 32000, 0), x)
        assert _convert_guarded(e, x, 32000, 1).tobytes() == A.to_pcm16(x)
        assert np.array_equal(_convert_guarded(e, x, 0, 0), x)       # rate 0 means 32000


def test_bad_rate_and_format_are_refused():
    import torch
    from genie_tts_amd.engine import _stream, lib
    e = _engine("v2")
    x = torch.zeros(64, device=e.dev)
    out = torch.zeros(256, device=e.dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for bad in O.BAD_RATES:
        assert lib().gsv_audio_convert(e.h, p(x), 64, bad, 0, p(out), _stream()) == -1
        with pytest.raises(ValueError):
            e.audio_convert(x, bad)
    for fmt in (-1, 2):
        assert lib().gsv_audio_convert(e.h, p(x), 64, 16000, fmt, p(out), _stream()) == -1
    txt, sem = _utt(8, 10)
    item, keep, res = e._vits_item(dict(text_seq=txt, pred_semantic=sem, sample_rate=16000, **_cond("v2")))
    for rate, fmt in ((12345, 0), (16000, 2)):                      # GSV_E_ARG before any launch
        item.out_rate, item.out_format = rate, fmt
        assert lib().gsv_vits_decode_item(e.h, ctypes.byref(item), ctypes.c_float(0.5), _stream()) == -1
        assert lib().gsv_vits_decode_batch(e.h, 1, ctypes.byref(item), ctypes.c_float(0.5), _stream()) == -1
    with pytest.raises(ValueError):
        e.vits_decode(txt, sem, sample_rate=12345, **_cond("v2"))


# ------------------------------------------------------------------ through the vocoder
def _cond(ver):
    if ver == "v2":
        return dict(ref_audio=synth.synth_ref_audio(32000 * 2 + 1234))
    return dict(ge=synth.synth_ge(1024), ge_advanced=synth.synth_ge(512, "adv"))


def _utt(G, S, tag="sr"):
    txt = synth.synth_phones(S, f"{tag}{S}")
    sem = ((np.arange(G, dtype=np.int64) * 37 + 11) % 1024).reshape(1, 1, G)
    return txt, sem


def _two_utts(e, ver):
    """G = 16, S = 12 at speed 1 with eps, and a second utterance at speed 1.25."""
    kw = _cond(ver)
    txt, sem = _utt(16, 12)
    eps = synth.rng_for("sr-eps").standard_normal((1, 192, 32)).astype(np.float32)
    txt2, sem2 = _utt(21, 9, "srb")
    return [dict(text_seq=txt, pred_semantic=sem, eps=eps, **kw),
            dict(text_seq=txt2, pred_semantic=sem2, speed=1.25, **kw)]


def _same_as_convert(e, out, a32, rate, pcm, what):
    """`out` is audio_convert of the same call's 32 kHz audio, bit for bit."""
    from genie_tts_amd.engine import audio_samples
    import torch
    assert out.dtype == (torch.int16 if pcm else torch.float32), what
    assert out.shape == (audio_samples(a32.numel(), rate),), what
    want = e.audio_convert(a32, rate, pcm16=pcm)
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy()), what


def test_vits_decode_at_a_rate(setup):
    ver, e = setup
    for it in _two_utts(e, ver):
        speed = it.get("speed", 1.0)
        kw = {k: v for k, v in it.items() if k not in ("text_seq", "pred_semantic", "speed")}
        plain = e.vits_decode(it["text_seq"], it["pred_semantic"], speed=speed, **kw).cpu().numpy()
        for rate in (8000, 44100, 48000):
            out = e.vits_decode(it["text_seq"], it["pred_semantic"], speed=speed, sample_rate=rate, **kw)
            a32 = e.vits_audio_32k[0]
            assert np.array_equal(a32.cpu().numpy(), plain)          # the 32 kHz audio is still written, unchanged
            _same_as_convert(e, out, a32, rate, False, (ver, speed, rate))
            err = float(np.abs(out.cpu().numpy().astype(np.float64) - O.resample(plain, rate)).max())
            print(f"{ver} speed {speed} {rate} Hz: max abs err {err:.2e}")
            assert err <= BOUND
        out = e.vits_decode(it["text_seq"], it["pred_semantic"], speed=speed, pcm16=True, **kw)
        _same_as_convert(e, out, e.vits_audio_32k[0], 32000, True, (ver, speed, "pcm16"))


def _mixed_batch(e, ver):
    a, b = _two_utts(e, ver)
    c = dict(a, eps=None, noise_seed=77)
    return [dict(a, sample_rate=8000), dict(b, sample_rate=32000, pcm16=True), dict(c, sample_rate=44100)], \
        [(8000, False), (32000, True), (44100, False)]


@pytest.mark.parametrize("seg", [0, 1])
def test_batch_with_mixed_rates(setup, seg):
    """8000 / 32000-pcm16 / 44100 in one batch, under seg_vocoder 0 and 1, synchronous and
    through _batch_async: each `out` is the conversion of that item's own `audio`."""
    ver, e = setup
    items, fmts = _mixed_batch(e, ver)
    e.set_option("seg_vocoder", seg)
    try:
        outs = e.vits_decode_batch(items)
        a32 = list(e.vits_audio_32k)
        for i, (rate, pcm) in enumerate(fmts):
            _same_as_convert(e, outs[i], a32[i], rate, pcm, (ver, seg, "sync", i))
        plain = e.vits_decode_batch([{k: v for k, v in it.items() if k not in ("sample_rate", "pcm16")}
                                     for it in items])
        for i in range(3):                                           # ... which the fields did not move
            assert np.array_equal(a32[i].cpu().numpy(), plain[i].cpu().numpy()), (ver, seg, i)
        outs = e.vits_decode_batch_async(items)
        a32 = list(e.vits_audio_32k)
        e.vits_batch_wait()
        for i, (rate, pcm) in enumerate(fmts):
            _same_as_convert(e, outs[i], a32[i], rate, pcm, (ver, seg, "async", i))
            assert np.array_equal(a32[i].cpu().numpy(), plain[i].cpu().numpy()), (ver, seg, "async", i)
    finally:
        e.set_option("seg_vocoder", 1)


def test_overlapped_call_on_the_vocoder_cus(setup):
    ver, e = setup
    items, fmts = _mixed_batch(e, ver)
    e.set_vocoder_cus(64)
    try:
        for it, (rate, pcm) in zip(items, fmts):
            out = e.vits_decode_async(it)
            a32 = e.vits_audio_32k[0]
            e.vits_wait()
            _same_as_convert(e, out, a32, rate, pcm, (ver, rate))
    finally:
        e.set_vocoder_cus(0)


def test_fp16_range_rerun_converts_the_reruns_audio(setup):
    """test_vits_gpu.py's recipe (eps x 1e6): `out` is the conversion of the re-run's audio."""
    ver, e = setup
    it = _two_utts(e, ver)[0]
    eps = (synth.rng_for("sr-big").standard_normal((1, 192, 32)) * 1e6).astype(np.float32)
    kw = {k: v for k, v in it.items() if k not in ("text_seq", "pred_semantic", "eps")}
    e.set_option("convh", 0)
    try:
        f32 = e.vits_decode(it["text_seq"], it["pred_semantic"], eps=eps, **kw).cpu().numpy()
    finally:
        e.set_option("convh", 1)
    n0 = e.counter("vits_f32_reruns")
    out = e.vits_decode(it["text_seq"], it["pred_semantic"], eps=eps, sample_rate=44100, pcm16=True, **kw)
    assert e.counter("vits_f32_reruns") == n0 + 1
    a32 = e.vits_audio_32k[0]
    assert np.array_equal(a32.cpu().numpy(), f32)
    _same_as_convert(e, out, a32, 44100, True, (ver, "rerun"))
    e.set_vocoder_cus(64)
    try:
        out = e.vits_decode_async(dict(it, eps=eps, sample_rate=8000))
        a32 = e.vits_audio_32k[0]
        e.vits_wait()
    finally:
        e.set_vocoder_cus(0)
    assert e.counter("vits_f32_reruns") == n0 + 2
    assert np.array_equal(a32.cpu().numpy(), f32)
    _same_as_convert(e, out, a32, 8000, False, (ver, "async rerun"))


# ------------------------------------------------------------------ top level
def test_api_tts_and_stream_at_a_rate(monkeypatch):
    """tts_stream of two sentences at 16 kHz equals the two single tts calls at 16 kHz;
    sample_rate=32000 equals the call without it; the default call equals itself."""
    import os
    import genie_tts_amd as G
    from genie_tts_amd import api
    from genie_tts_amd.engine import audio_samples, make_sampler
    from genie_tts_amd.model_manager import build_model, model_manager
    from tests.test_api_gpu import GOLD, _eos_character
    div = np.load(os.path.join(GOLD, "pe_div_term.npy"))
    m = build_model(_eos_character(), "v2", sampler=make_sampler(greedy=True), pe_div_term=div)
    m.VITS.noise = "zero"
    sp = m.T2S_FIRST_STAGE_DECODER.sampler
    try:
        model_manager._put("rate_char", m)
        model_manager.character_to_language["rate_char"] = "Japanese"
        G.set_reference_features("rate_char", synth.synth_phones(12, "sra-r"), None,
                                 synth.synth_ref_audio(32000 * 2, "sra-a"), synth.synth_ssl(41, "sra-s"))
        texts = [synth.synth_phones(10, "sra-t0"), synth.synth_phones(17, "sra-t1")]
        cur = []
        monkeypatch.setattr(api, "_sentences", lambda text, split: list(cur))
        seen = []
        real = m.ENGINE.vits_decode_async
        monkeypatch.setattr(m.ENGINE, "vits_decode_async",
                            lambda item, scale=0.5: (seen.append(item.get("sample_rate")), real(item, scale))[1])
        cur[:] = texts
        plain = G.tts("rate_char", None, sampler=sp)
        assert np.array_equal(G.tts("rate_char", None, sampler=sp), plain)      # nothing moved
        assert seen == [None] * 4
        assert np.array_equal(G.tts("rate_char", None, sampler=sp, sample_rate=32000), plain)
        stream = G.tts("rate_char", None, sampler=sp, sample_rate=16000)
        assert seen[-2:] == [16000, 16000]
        singles = []
        for t in texts:
            cur[:] = [t]
            singles.append(G.tts("rate_char", None, sampler=sp, sample_rate=16000))
            p32 = G.tts("rate_char", None, sampler=sp)
            assert singles[-1].dtype == np.float32 and singles[-1].shape == (audio_samples(p32.size, 16000),)
            assert np.abs(singles[-1].astype(np.float64) - O.resample(p32, 16000)).max() <= BOUND
        assert np.array_equal(stream, np.concatenate(singles))

        async def go(**kw):
            return [c async for c in api.tts_async("rate_char", None, sampler=sp, **kw)]
        cur[:] = [texts[0]]
        assert asyncio.run(go(sample_rate=32000)) == asyncio.run(go())            # the GPU's int16 = to_pcm16
        c48 = asyncio.run(go(sample_rate=48000))
        p32 = G.tts("rate_char", None, sampler=sp)
        assert c48 == [m.ENGINE.audio_convert(p32, 48000, pcm16=True).cpu().numpy().tobytes()]
    finally:
        model_manager.character_to_model.pop("rate_char", None)
        api.clear_reference_audio_cache()
        m.ENGINE.close()


def test_server_round_with_two_rates(tmp_path):
    """test_server_gpu.py's set-up: requests at 8 kHz and 48 kHz and one without the field, sent
    together.  Each gets its own rate's samples and X-Sample-Rate; the one without gets the
    32 kHz host-converted stream with no header, bit-equal to the same request sent again.

    The rated streams are checked against the oracle applied to the plain stream p0 (int16 at
    32 kHz) of the same text.  Bound, in int16 steps: the three utterances may share a segmented
    batch, where an utterance matches itself alone within 1e-4 (test_vits_gpu.py's rule), so two
    positions differ by <= 2e-4 * 32767 = 6.6; p0 is truncated (+ 1); the filter grows that by
    sum|h| <= 2.25; the float32 chain adds 0.39 and the output truncation 1: (6.6 + 1) * 2.25 +
    1.39 = 18.5 -> 19."""
    import httpx
    from genie_tts_amd.server import Router, create_app
    wav = str(tmp_path / "ref.wav")
    x = (0.1 * np.random.default_rng(1).standard_normal(4 * 32000)).clip(-1, 1)
    with wave.open(wav, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(32000)
        wf.writeframes((x * 32767).astype("<i2").tobytes())
    text, G = "ありがとうございます。", 24
    saved = str(tmp_path / "out48.wav")

    async def run():
        router = Router([0], g2p="genie_tts_amd.stubs:toy_g2p", ssl="genie_tts_amd.stubs:toy_ssl", greedy=True,
                        noise="zero")
        router.start(asyncio.get_running_loop(), timeout=300)
        try:
            res = await router.broadcast("load_synthetic", character_name="srv", version="v2")
            assert all(r["kind"] == "ok" for r in res), res
            tr = httpx.ASGITransport(app=create_app(router))
            async with httpx.AsyncClient(transport=tr, base_url="http://t", timeout=300) as cl:
                r = await cl.post("/set_reference_audio", json=dict(character_name="srv", audio_path=wav,
                                                                    audio_text="こんにちは。", language="ja"))
                assert r.status_code == 200, r.text

                async def one(**kw):
                    r = await cl.post("/tts", json=dict(character_name="srv", text=text, force_steps=G + 1, **kw))
                    assert r.status_code == 200, r.text
                    return r
                r8, r48, r0 = await asyncio.gather(one(sample_rate=8000), one(sample_rate=48000, save_path=saved),
                                                   one())
                again = await one()
                again2 = await one()
                return r8, r48, r0, again, again2
        finally:
            router.close()
    r8, r48, r0, again, again2 = asyncio.run(run())
    assert r8.headers["x-sample-rate"] == "8000" and r48.headers["x-sample-rate"] == "48000"
    assert "x-sample-rate" not in r0.headers and "x-sample-rate" not in again.headers
    p0 = np.frombuffer(r0.content, np.int16)
    assert p0.size == 1280 * G and np.abs(p0).max() > 100
    assert again.content == again2.content and len(again.content) == len(r0.content)
    for r, rate in ((r8, 8000), (r48, 48000)):
        got = np.frombuffer(r.content, np.int16).astype(np.float64)
        want = np.clip(O.resample(p0 / 32767.0, rate) * 32767.0, -32768.0, 32767.0)
        assert got.shape == want.shape == (O.n_out(1280 * G, rate),)
        err = float(np.abs(got - want).max())
        print(f"server {rate} Hz: max |got - oracle(p0)| {err:.2f} int16 steps, peak {np.abs(got).max():.0f}")
        assert err <= 19
    with wave.open(saved) as f:                                     # the streamed samples, the header at their rate
        assert f.getframerate() == 48000 and f.readframes(f.getnframes()) == r48.content
