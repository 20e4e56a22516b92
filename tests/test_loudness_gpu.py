"""GPU: the loudness stage (ITU-R BS.1770-4 target under a peak ceiling; include/genie_engine.h,
gsv_loudness) -- the filter and its carry alone against the float64 oracle
(tests/loudness_oracle.py, pinned by tests/test_loudness_host.py), the gate, the gain, the gain
applied by the output stage, behind every vocoder entry point, and from api.tts / the server down.

Bounds.  Hop energies: |e - e64| <= tol * e64 + 1e-7 * max_k e64_k (the second term: a silent hop
behind a loud one holds float32 rounding residue only).  tol is 8 x the same figure of the
sequential float32 form on the CPU (scipy.signal.lfilter on float32 arrays) for that input, at
least 2e-4 (3200 float32 additions).  Loudness: 0.1 LU (EBU Tech 3341's meter tolerance), on
signals whose every block the oracle puts >= 0.5 LU from both gates, so blocks_kept is equal;
the peak is bit-equal.  Gain: 1e-5 relative of the formula in float64 on the float32 loudness
and peak.  Applying: float32(convert(audio)) * float32(gain), bit for bit, then the int16 rule.
Measured figures: DESIGN §4.3d.
"""
import asyncio
import ctypes
import math
import wave

import numpy as np
import pytest

from genie_tts_amd import synth
from tests import loudness_oracle as O
from tests.test_sample_rate_gpu import _cond, _two_utts, _utt

pytestmark = pytest.mark.gpu

SHORT = (1, 3199, 3200, 3201, 12799, 12800, 12801, 16000)
IMPULSES = (0, 3199, 3200, 6399)
_engines = {}
_ref = {}


def _engine(ver):
    from genie_tts_amd.engine import Engine
    from tests.common import character
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


def _inputs():
    """name -> float32 signal: the short sizes (uniform noise), the four signals, the impulses."""
    if not _ref:
        for n in SHORT:
            _ref[f"n{n}"] = (0.5 * np.random.default_rng(n).uniform(-1, 1, n)).astype(np.float32)
        _ref.update(O.signals())
        for at in IMPULSES:
            x = np.zeros(16000, np.float32)
            x[at] = 1.0
            _ref[f"impulse{at}"] = x
    return _ref


def _metric(e, e64):
    """The least tol with |e - e64| <= tol * e64 + 1e-7 * max e64 in every hop (inf: a silent hop misses)."""
    if e64.size == 0:
        return 0.0
    d = np.abs(np.asarray(e, np.float64) - e64) - 1e-7 * e64.max()
    if (d[e64 == 0] > 0).any():
        return math.inf
    nz = e64 > 0
    return float(np.maximum(d[nz] / e64[nz], 0.0).max()) if nz.any() else 0.0


def _stats(e, x, target=None, peak=None, rate=32000, pcm=False):
    """(stats float32 [4], out) of audio_loudness (target None) or audio_convert with a target."""
    if target is None:
        e.audio_loudness(x)
        return e.vits_loudness[0].cpu().numpy(), None
    out = e.audio_convert(x, rate, pcm16=pcm, loudness=target, peak=peak)
    return e.vits_loudness[0].cpu().numpy(), out


def test_hop_energies_against_the_oracle():
    e = _engine("v2")
    worst = 0.0
    for name, x in _inputs().items():
        e64 = O.hops(x)
        got = e.debug_loudness_hops(x).cpu().numpy()
        assert got.shape == e64.shape == (x.size // 3200,), name
        cpu = _metric(O.hops(x, dtype=np.float32), e64)
        tol = max(8.0 * cpu, 2e-4)
        fig = _metric(got, e64)
        worst = max(worst, fig)
        print(f"{name}: {e64.size} hops, float32 sequential {cpu:.2e}, GPU {fig:.2e} (tol {tol:.2e})")
        assert fig <= tol, (name, fig, tol)
    x = _inputs()["impulse3199"]                                    # hop 1 holds carried state alone
    assert abs(O.hops(x)[1] - 0.0832) < 1e-4
    print(f"hop energies: worst GPU figure {worst:.2e}")


def test_hop_energies_do_not_depend_on_the_grid():
    """An item gives the same bits alone and behind others in its buffer: `long` measured from
    offset 0 and as the tail of a longer buffer (another base alignment, the same hops)."""
    import torch
    e = _engine("v2")
    x = _inputs()["long"]
    alone = e.debug_loudness_hops(x).cpu().numpy()
    buf = torch.from_numpy(np.concatenate([np.ones(3, np.float32), x])).to(e.dev)
    assert np.array_equal(e.debug_loudness_hops(buf[3:]).cpu().numpy(), alone)
    assert np.array_equal(e.debug_loudness_hops(x).cpu().numpy(), alone)


def test_loudness_peak_and_blocks_against_the_oracle():
    e = _engine("v2")
    worst = 0.0
    for name, x in _inputs().items():
        if name.startswith("impulse"):
            continue
        m = O.measure(x)
        assert O.gate_margin(x) >= 0.5, name                         # on the oracle alone
        st, _ = _stats(e, x)
        err = abs(float(st[0]) - m["loudness"])
        worst = max(worst, err)
        print(f"{name}: oracle {m['loudness']:.4f} LUFS, GPU {st[0]:.4f}, kept {int(st[3])} of {m['blocks']}")
        assert err <= 0.1, (name, st[0], m["loudness"])
        assert int(st[3]) == m["blocks_kept"], name
        assert st[1] == np.abs(x).max() and st[1].dtype == np.float32, name
        assert st[2] == 1.0                                          # measuring alone: no gain
        lufs, pk = e.audio_loudness(x)
        assert (np.float32(lufs), np.float32(pk)) == (st[0], st[1])
    print(f"loudness: worst |GPU - oracle| {worst:.2e} LU")


def test_gain_formula_ceiling_and_silence():
    e = _engine("v2")
    x = _inputs()["steady"]
    hit = 0
    for name, target, peak in (("steady", -16.0, None), ("steady", -5.0, None), ("steady", -5.0, 0.5),
                               ("speech", -23.0, 1.0), ("n3201", -16.0, None)):
        x = _inputs()[name]
        st, _ = _stats(e, x, target, peak)
        loud = 10.0 ** ((target - float(st[0])) / 20.0)
        ceil = (peak or O.DEFAULT_PEAK) / float(st[1])
        want = min(loud, ceil)
        hit += ceil < loud
        print(f"{name} -> {target} LUFS, ceiling {peak}: gain {st[2]:.6f}, formula {want:.6f}"
              f" ({'ceiling' if ceil < loud else 'target'})")
        assert abs(float(st[2]) - want) <= 1e-5 * want, (name, target, peak)
        assert abs(want - O.gain(float(st[0]), float(st[1]), target, peak)) <= 1e-12 * want
    assert hit >= 1                                                  # the ceiling branch was taken
    for x in (np.zeros(16000, np.float32), np.zeros(5, np.float32), np.zeros(0, np.float32)):
        st, out = _stats(e, x, -16.0)
        assert st[0] == -np.inf and st[1] == 0 and st[2] == 1.0 and st[3] == 0, x.size
        assert np.array_equal(out.cpu().numpy(), x)
        st, _ = _stats(e, x)
        assert st[0] == -np.inf and st[2] == 1.0 and st[3] == 0, x.size


def _normalize_guarded(e, x, target, peak, rate, fmt):
    """gsv_audio_normalize into a sentinel-filled buffer with one guard element past n_out."""
    import torch
    from genie_tts_amd.engine import _check, _stream, lib
    n_out = lib().gsv_audio_samples(x.size, rate)
    xd = torch.from_numpy(x).to(e.dev)
    stats = torch.full((5,), 777.0, dtype=torch.float32, device=e.dev)
    if fmt == 0:
        out = torch.full((n_out + 1,), float("nan"), dtype=torch.float32, device=e.dev)
    else:
        out = torch.full((n_out + 1,), -12345, dtype=torch.int16, device=e.dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _check(lib().gsv_audio_normalize(e.h, p(xd), x.size, ctypes.c_float(target), ctypes.c_float(peak), rate, fmt,
                                     p(out), p(stats), _stream()), "gsv_audio_normalize")
    got, st = out.cpu().numpy(), stats.cpu().numpy()
    assert np.isnan(got[-1]) if fmt == 0 else got[-1] == -12345, "the guard element was written"
    assert st[4] == 777.0
    return got[:-1], st[:4]


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_gain_applied_by_the_output_stage(rate):
    e = _engine("v2")
    for name, target in (("steady", -20.0), ("long", -16.0), ("n3201", -9.0)):
        x = _inputs()[name]
        plain = e.audio_convert(x, rate).cpu().numpy()
        got, st = _normalize_guarded(e, x, target, 0.0, rate, 0)
        want = plain.astype(np.float32) * np.float32(st[2])
        assert st[2] != 1.0 and np.array_equal(got, want), (name, rate)
        pcm, st2 = _normalize_guarded(e, x, target, 0.0, rate, 1)
        assert np.array_equal(st, st2)
        v = np.clip(want * np.float32(32767.0), np.float32(-32768.0), np.float32(32767.0))
        assert v.dtype == np.float32 and np.array_equal(pcm, np.trunc(v).astype(np.int16)), (name, rate)
        assert np.array_equal(e.audio_convert(x, rate, loudness=target).cpu().numpy(), got)   # the Python binding
        assert np.array_equal(e.audio_convert(x, rate).cpu().numpy(), plain)                  # and nothing moved


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from genie_tts_amd.engine import Loudness, _stream, lib
    e = _engine("v2")
    x = torch.zeros(6400, device=e.dev)
    out = torch.zeros(9600, device=e.dev)
    st = torch.zeros(4, device=e.dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = ctypes.c_float
    L = lib()
    bad = [(t, 0.0) for t in (0.0, -4.9, -50.1, 3.0, float("nan"), float("inf"))] + \
          [(-16.0, pk) for pk in (-0.1, 1.01, float("nan"))]
    for target, peak in bad:
        assert L.gsv_audio_normalize(e.h, p(x), 6400, f(target), f(peak), 48000, 0, p(out), p(st), _stream()) == -1
    assert L.gsv_audio_normalize(e.h, p(x), 6400, f(-16.0), f(0.0), 12345, 0, p(out), p(st), _stream()) == -1
    assert L.gsv_audio_normalize(e.h, p(x), 6400, f(-16.0), f(0.0), 48000, 2, p(out), p(st), _stream()) == -1
    assert L.gsv_audio_loudness(e.h, p(x), -1, p(st), _stream()) == -1
    assert L.gsv_audio_loudness(e.h, p(x), 640 * 4096 + 1, p(st), _stream()) == -1
    for v in (-4.0, -51.0, 0, 0.0, True, "loud", float("nan")):
        with pytest.raises(ValueError):
            e.audio_convert(x, 48000, loudness=v)
    for v in (0.0, -0.5, 1.5, "1", float("nan")):
        with pytest.raises(ValueError):
            e.audio_convert(x, 48000, loudness=-16.0, peak=v)
    txt, sem = _utt(8, 10)
    call = e._vocoder_call([dict(text_seq=txt, pred_semantic=sem, loudness=-16.0, **_cond("v2"))])
    item, spec = call.items[0], call.specs[0]
    ld = Loudness(spec.target, spec.peak, spec.stats)                # the `_norm` entries' form of the item's spec
    assert item.out and ld.target == -16.0
    entries = (lambda: L.gsv_vits_decode_item_norm(e.h, ctypes.byref(item), ctypes.byref(ld), f(0.5), _stream()),
               lambda: L.gsv_vits_decode_batch_norm(e.h, 1, ctypes.byref(item), ctypes.byref(ld), f(0.5), _stream()),
               lambda: L.gsv_vits_decode_batch_async_norm(e.h, 1, ctypes.byref(item), ctypes.byref(ld), f(0.5),
                                                          _stream()),
               lambda: L.gsv_vits_decode_async_norm(e.h, ctypes.byref(item), ctypes.byref(ld), f(0.5), _stream()))
    for target, peak in bad[1:]:
        ld.target, ld.peak = target, peak
        assert [fn() for fn in entries] == [-1] * 4, (target, peak)
    ld.target, ld.peak = -16.0, 0.0
    out_ptr, item.out = item.out, None                               # a target without `out`
    assert [fn() for fn in entries] == [-1] * 4
    item.out = out_ptr
    with pytest.raises(ValueError):
        e.vits_decode(txt, sem, loudness=-4.0, **_cond("v2"))
    with pytest.raises(ValueError):
        e.vits_decode_batch([dict(text_seq=txt, pred_semantic=sem, loudness=-16.0, peak=2.0, **_cond("v2"))])
    assert isinstance(Loudness(), ctypes.Structure)


# ------------------------------------------------------------------ through the vocoder
def _same_as_normalize(e, out, stats, a32, rate, pcm, target, peak, what):
    """`out` and `stats` are gsv_audio_normalize of the same call's 32 kHz audio, bit for bit."""
    import torch
    from genie_tts_amd.engine import audio_samples
    assert out.dtype == (torch.int16 if pcm else torch.float32), what
    assert out.shape == (audio_samples(a32.numel(), rate or 32000),), what
    got, st = out.cpu().numpy(), stats.cpu().numpy()
    want = e.audio_convert(a32, rate or 32000, pcm16=pcm, loudness=target, peak=peak)
    assert np.array_equal(st, e.vits_loudness[0].cpu().numpy()), (what, st)
    assert np.array_equal(got, want.cpu().numpy()), what
    assert st[2] != 1.0 and st[3] > 0 and np.isfinite(st[0]), (what, st)


def _plain(it):
    return {k: v for k, v in it.items() if k not in ("sample_rate", "pcm16", "loudness", "peak")}


def test_vits_decode_normalised(setup):
    ver, e = setup
    for it in _two_utts(e, ver):
        speed = it.get("speed", 1.0)
        kw = {k: v for k, v in it.items() if k not in ("text_seq", "pred_semantic", "speed")}
        plain = e.vits_decode(it["text_seq"], it["pred_semantic"], speed=speed, **kw).cpu().numpy()
        for rate, pcm, peak in ((None, False, None), (48000, True, 0.5), (8000, False, None)):
            out = e.vits_decode(it["text_seq"], it["pred_semantic"], speed=speed, sample_rate=rate, pcm16=pcm,
                                loudness=-16.0, peak=peak, **kw)
            a32, st = e.vits_audio_32k[0], e.vits_loudness[0]
            assert np.array_equal(a32.cpu().numpy(), plain)          # the 32 kHz audio: written, unnormalised
            _same_as_normalize(e, out, st, a32, rate, pcm, -16.0, peak, (ver, speed, rate))


@pytest.mark.parametrize("seg", [0, 1])
def test_batch_with_one_normalised_and_one_plain_item(setup, seg):
    ver, e = setup
    a, b = _two_utts(e, ver)
    items = [dict(a, sample_rate=44100, pcm16=True, loudness=-18.0), dict(b, sample_rate=8000)]
    e.set_option("seg_vocoder", seg)
    try:
        old = e.vits_decode_batch([_plain(items[0]), items[1]])
        old32 = [t.cpu().numpy() for t in e.vits_audio_32k]
        old1 = old[1].cpu().numpy()
        for mode in ("sync", "async"):
            outs = e.vits_decode_batch(items) if mode == "sync" else e.vits_decode_batch_async(items)
            a32, st = list(e.vits_audio_32k), list(e.vits_loudness)
            if mode == "async":
                e.vits_batch_wait()
            assert st[1] is None
            for i in range(2):                                       # the keywords did not move the 32 kHz audio
                assert np.array_equal(a32[i].cpu().numpy(), old32[i]), (ver, seg, mode, i)
            assert np.array_equal(outs[1].cpu().numpy(), old1), (ver, seg, mode)   # the plain item: its old result
            _same_as_normalize(e, outs[0], st[0], a32[0], 44100, True, -18.0, None, (ver, seg, mode))
    finally:
        e.set_option("seg_vocoder", 1)


def test_overlapped_call_on_the_vocoder_cus(setup):
    ver, e = setup
    a, b = _two_utts(e, ver)
    e.set_vocoder_cus(64)
    try:
        for it, rate, pcm in ((dict(a, loudness=-16.0), None, False),
                              (dict(b, sample_rate=48000, pcm16=True, loudness=-20.0, peak=0.7), 48000, True)):
            out = e.vits_decode_async(it)
            a32, st = e.vits_audio_32k[0], e.vits_loudness[0]
            e.vits_wait()
            _same_as_normalize(e, out, st, a32, rate, pcm, it["loudness"], it.get("peak"), (ver, rate))
        out = e.vits_decode_async(dict(b, sample_rate=8000))         # a plain call behind them: today's
        assert e.vits_loudness == [None]
        a32 = e.vits_audio_32k[0]
        e.vits_wait()
        assert np.array_equal(out.cpu().numpy(), e.audio_convert(a32, 8000).cpu().numpy())
    finally:
        e.set_vocoder_cus(0)


def test_fp16_range_rerun_measures_the_reruns_audio(setup):
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
    out = e.vits_decode(it["text_seq"], it["pred_semantic"], eps=eps, sample_rate=44100, pcm16=True, loudness=-16.0,
                        **kw)
    assert e.counter("vits_f32_reruns") == n0 + 1
    a32, st = e.vits_audio_32k[0], e.vits_loudness[0]
    assert np.array_equal(a32.cpu().numpy(), f32)
    _same_as_normalize(e, out, st, a32, 44100, True, -16.0, None, (ver, "rerun"))
    e.set_vocoder_cus(64)
    try:
        out = e.vits_decode_async(dict(it, eps=eps, loudness=-16.0))
        a32, st = e.vits_audio_32k[0], e.vits_loudness[0]
        e.vits_wait()
    finally:
        e.set_vocoder_cus(0)
    assert e.counter("vits_f32_reruns") == n0 + 2
    assert np.array_equal(a32.cpu().numpy(), f32)
    _same_as_normalize(e, out, st, a32, None, False, -16.0, None, (ver, "async rerun"))


def test_methods_without_a_target_give_the_plain_entries_bits(setup):
    """The Engine's vocoder methods call the `_join` entries whether or not an item has a target.
    Without one, each returns the bits of a direct call of the plain C entry on the same item
    (G = 8, 3 text ids, Philox noise from one seed), as float32 at 32 kHz and as int16 at 16 kHz.
    vits_decode takes the batch entry with a seed and the item entry without one (zero noise)."""
    import torch
    from genie_tts_amd.engine import _check, _stream, lib
    ver, e = setup
    L, f = lib(), ctypes.c_float(0.5)
    txt, sem = _utt(8, 3)
    seeded = dict(text_seq=txt, pred_semantic=sem, noise_seed=7, **_cond(ver))
    unseeded = {k: v for k, v in seeded.items() if k != "noise_seed"}

    def kwargs(it):
        return {k: v for k, v in it.items() if k not in ("text_seq", "pred_semantic")}

    def wait(out, fn):
        fn()
        return out
    routes = (
        ("vits_decode, seed", seeded, lambda it: e.vits_decode(txt, sem, **kwargs(it)),
         lambda item: L.gsv_vits_decode_batch(e.h, 1, ctypes.byref(item), f, _stream())),
        ("vits_decode, no seed", unseeded, lambda it: e.vits_decode(txt, sem, **kwargs(it)),
         lambda item: L.gsv_vits_decode_item(e.h, ctypes.byref(item), f, _stream())),
        ("vits_decode_batch", seeded, lambda it: e.vits_decode_batch([it])[0],
         lambda item: L.gsv_vits_decode_batch(e.h, 1, ctypes.byref(item), f, _stream())),
        ("vits_decode_batch_async", seeded, lambda it: wait(e.vits_decode_batch_async([it])[0], e.vits_batch_wait),
         lambda item: L.gsv_vits_decode_batch_async(e.h, 1, ctypes.byref(item), f, _stream()) or
         L.gsv_vits_batch_wait(e.h, _stream())),
        ("vits_decode_async", seeded, lambda it: wait(e.vits_decode_async(it), e.vits_wait),
         lambda item: L.gsv_vits_decode_async(e.h, ctypes.byref(item), f, _stream()) or
         L.gsv_vits_wait(e.h, _stream())))
    for what, base, method, entry in routes:
        if what == "vits_decode_async":                              # on its own CUs, as above
            e.set_vocoder_cus(64)
        try:
            for opts in ({}, dict(sample_rate=16000, pcm16=True)):
                it = dict(base, **opts)
                item, keep, want = e._vits_item(it)
                _check(entry(item), what)
                got = method(it)
                assert e.vits_loudness == [None], what
                assert got.dtype == want.dtype == (torch.int16 if opts else torch.float32), what
                assert got.shape == want.shape == ((640 * 8,) if opts else (1280 * 8,)), what
                assert torch.equal(got, want), (ver, what, opts)
                assert bool(want.any()), what                       # audio, not an untouched buffer
        finally:
            if e.vocoder_cus:
                e.set_vocoder_cus(0)
    audio = torch.empty(1280 * 8, device=e.dev)                      # ... and of gsv_vits_decode, the item-less entry
    c = {k: e._dev(v, torch.float32).reshape(-1) for k, v in _cond(ver).items()}
    ts, sm = e._ids(txt), e._ids(sem)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    ra = c.get("ref_audio")
    _check(L.gsv_vits_decode(e.h, p(ts), 3, p(sm), 8, p(ra), 0 if ra is None else ra.numel(), p(c.get("ge")),
                             p(c.get("ge_advanced")), None, f, p(audio), _stream()), "gsv_vits_decode")
    assert torch.equal(e.vits_decode(txt, sem, **_cond(ver)), audio)


# ------------------------------------------------------------------ top level
def test_api_tts_and_stream_normalised(monkeypatch):
    """tts of two sentences with loudness=-16 equals the two single calls; tts_async's chunks at
    48 kHz equal audio_convert of the plain call's audio; without the keywords nothing moved."""
    import os
    import genie_tts_amd as G
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    from genie_tts_amd.model_manager import build_model, model_manager
    from tests.test_api_gpu import GOLD, _eos_character
    div = np.load(os.path.join(GOLD, "pe_div_term.npy"))
    m = build_model(_eos_character(), "v2", sampler=make_sampler(greedy=True), pe_div_term=div)
    m.VITS.noise = "zero"
    sp = m.T2S_FIRST_STAGE_DECODER.sampler
    try:
        model_manager._put("loud_char", m)
        model_manager.character_to_language["loud_char"] = "Japanese"
        G.set_reference_features("loud_char", synth.synth_phones(12, "sra-r"), None,
                                 synth.synth_ref_audio(32000 * 2, "sra-a"), synth.synth_ssl(41, "sra-s"))
        texts = [synth.synth_phones(10, "sra-t0"), synth.synth_phones(17, "sra-t1")]
        cur = []
        monkeypatch.setattr(api, "_sentences", lambda text, split: list(cur))
        seen = []
        real = m.ENGINE.vits_decode_async
        monkeypatch.setattr(m.ENGINE, "vits_decode_async",
                            lambda item, scale=0.5: (seen.append(item.get("loudness")), real(item, scale))[1])
        cur[:] = texts
        plain = G.tts("loud_char", None, sampler=sp)
        stream = G.tts("loud_char", None, sampler=sp, loudness=-16)
        assert seen == [None, None, -16.0, -16.0]
        assert np.array_equal(G.tts("loud_char", None, sampler=sp), plain)      # nothing moved
        assert stream.dtype == np.float32 and stream.shape == plain.shape and not np.array_equal(stream, plain)
        singles = []
        for t in texts:
            cur[:] = [t]
            singles.append(G.tts("loud_char", None, sampler=sp, loudness=-16))
            p32 = G.tts("loud_char", None, sampler=sp)
            want = m.ENGINE.audio_convert(p32, 32000, loudness=-16).cpu().numpy()
            assert np.array_equal(singles[-1], want)
            st = m.ENGINE.vits_loudness[0].cpu().numpy()
            got = O.loudness(singles[-1])
            print(f"sentence of {p32.size} samples: {st[0]:.3f} LUFS, peak {st[1]:.3f}, gain {st[2]:.4f} -> "
                  f"{got:.3f} by the oracle")
        assert np.array_equal(stream, np.concatenate(singles))

        async def go(**kw):
            return [c async for c in api.tts_async("loud_char", None, sampler=sp, **kw)]
        cur[:] = [texts[0]]
        c48 = asyncio.run(go(loudness=-16, sample_rate=48000))
        p32 = G.tts("loud_char", None, sampler=sp)
        assert c48 == [m.ENGINE.audio_convert(p32, 48000, pcm16=True, loudness=-16).cpu().numpy().tobytes()]
        assert asyncio.run(go()) == asyncio.run(go(sample_rate=32000))            # as before
        with pytest.raises(ValueError):
            G.tts("loud_char", None, sampler=sp, loudness=-3)
    finally:
        model_manager.character_to_model.pop("loud_char", None)
        api.clear_reference_audio_cache()
        m.ENGINE.close()


def test_server_round_with_a_normalised_and_a_plain_request(tmp_path):
    """test_sample_rate_gpu.py's server set-up: a request with loudness=-16 and one without, sent
    together.  The plain one is byte-equal to itself sent alone; the normalised one measures
    -16 +- 0.2 LUFS by the oracle on its PCM: 0.1 for the meter plus the int16 truncation and the
    shared-batch slack of test_server_round_with_two_rates (both far below 0.1 LU)."""
    import httpx
    from genie_tts_amd.server import Router, create_app
    wav = str(tmp_path / "ref.wav")
    x = (0.1 * np.random.default_rng(1).standard_normal(4 * 32000)).clip(-1, 1)
    with wave.open(wav, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(32000)
        wf.writeframes((x * 32767).astype("<i2").tobytes())
    text, G = "ありがとうございます。", 24

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
                alone = await one()
                loud, plain = await asyncio.gather(one(loudness=-16, peak=1.0), one())
                bad = await cl.post("/tts", json=dict(character_name="srv", text=text, loudness=-3))
                return alone, loud, plain, bad
        finally:
            router.close()
    alone, loud, plain, bad = asyncio.run(run())
    assert bad.status_code == 400 and bad.json()["detail"].startswith("loudness:")
    assert loud.headers["x-loudness"] == "-16" and "x-loudness" not in plain.headers
    assert plain.content == alone.content and len(loud.content) == len(plain.content) == 2 * 1280 * G
    p0 = np.frombuffer(plain.content, np.int16) / 32767.0
    p1 = np.frombuffer(loud.content, np.int16) / 32767.0
    before, after = O.measure(p0), O.measure(p1)
    print(f"server: plain {before['loudness']:.3f} LUFS (peak {before['peak']:.3f}), normalised "
          f"{after['loudness']:.3f} LUFS (peak {after['peak']:.3f})")
    assert abs(after["loudness"] + 16.0) <= 0.2
