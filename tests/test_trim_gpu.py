"""GPU: the sentence join (edge-silence trim and pause; include/genie_engine.h, gsv_join) -- the
frame pass alone against the float64 oracle (tests/trim_oracle.py, pinned by
tests/test_trim_host.py), the span records, the output stage over a span, and every vocoder
entry point.

Bounds.  Frame sums: relative 1e-12 (320 non-negative doubles: any order is within 320 * 2^-53 =
3.6e-14).  Span records: the oracle's integers, on inputs where the oracle puts every frame's mean
square further than 1e-6 relative from the threshold (asserted on the oracle alone).  Output:
out[:n_speech] is Engine.audio_convert of audio[begin:end] bit for bit, the pause is zeros, and
nothing past n_out is written.
"""
import ctypes

import numpy as np
import pytest

from genie_tts_amd import synth
from tests import trim_oracle as O
from tests.test_sample_rate_gpu import _cond, _utt

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 319, 320, 321, 959, 6400, 40000)
TRIM = -50.0
_engines = {}
_sig = {}


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


def _level(n, db, seed):
    """Uniform noise whose every frame has a mean square `db` dB from the threshold."""
    x = np.random.default_rng(seed).uniform(-1, 1, n)
    want = O.threshold(TRIM) * 10.0 ** (db / 10.0)
    for f in range((n + O.FRAME - 1) // O.FRAME):
        s = x[f * O.FRAME:(f + 1) * O.FRAME]
        s *= np.sqrt(want / np.mean(s ** 2))
    return x.astype(np.float32)


def _signals():
    """(n, kind) -> float32 signal, built once: every kind the length allows."""
    if _sig:
        return _sig
    for n in LENGTHS:
        rng = np.random.default_rng(n + 1)
        speech = (0.3 * rng.uniform(-1, 1, n)).astype(np.float32)
        part = max(1, n // 3)
        _sig[n, "silent"] = np.zeros(n, np.float32)
        if n == 0:
            continue
        x = np.zeros(n, np.float32)
        x[:part] = speech[:part]
        _sig[n, "from0"] = x                                         # the guard clips at 0
        x = np.zeros(n, np.float32)
        x[n - part:] = speech[n - part:]
        _sig[n, "to_end"] = x
        nf = (n + O.FRAME - 1) // O.FRAME
        if n % O.FRAME:
            x = np.zeros(n, np.float32)
            x[(nf - 1) * O.FRAME:] = 0.5
            _sig[n, "partial_last"] = x
        if n >= 2 * O.FRAME:
            x = np.zeros(n, np.float32)
            f = nf // 2 if n % O.FRAME == 0 or nf // 2 < nf - 1 else 0
            x[f * O.FRAME:(f + 1) * O.FRAME] = speech[f * O.FRAME:(f + 1) * O.FRAME]
            _sig[n, "single_frame"] = x
        x = (1e-4 * rng.uniform(-1, 1, n)).astype(np.float32)        # -85 dBFS under ...
        x[n // 2] = 0.9                                              # ... a click
        _sig[n, "click"] = x
        _sig[n, "noise+1dB"] = _level(n, 1.0, n + 7)
        _sig[n, "noise-1dB"] = _level(n, -1.0, n + 9)
    return _sig


def _join_guarded(e, x, rate=32000, fmt=0, pause=0.0, trim=0.0, target=0.0, pad=300):
    """gsv_audio_join into a buffer pre-filled with a sentinel, `pad` elements past the bound.
    -> (the whole buffer, the span record, stats or None)."""
    import torch
    from genie_tts_amd.engine import Join, _check, _stream, lib
    bound = lib().gsv_join_samples(x.size, rate, ctypes.c_float(pause))
    assert bound == O.audio_samples(x.size, rate or 32000) + O.pause_samples(rate or 32000, pause)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(e.dev)
    if fmt == 0:
        out = torch.full((bound + pad,), float("nan"), dtype=torch.float32, device=e.dev)
    else:
        out = torch.full((bound + pad,), -12345, dtype=torch.int16, device=e.dev)
    span = torch.full((4,), -7, dtype=torch.int32, device=e.dev)
    stats = torch.zeros(4, dtype=torch.float32, device=e.dev) if target else None
    j = Join(target, 0.0, stats.data_ptr() if target else None, trim, pause, span.data_ptr())
    _check(lib().gsv_audio_join(e.h, ctypes.c_void_p(xd.data_ptr()), x.size, ctypes.byref(j), rate, fmt,
                                ctypes.c_void_p(out.data_ptr()), _stream()), "gsv_audio_join")
    return out.cpu().numpy(), tuple(int(v) for v in span.cpu()), None if stats is None else stats.cpu().numpy()


def _untouched(buf, fmt):
    return np.isnan(buf).all() if fmt == 0 else (buf == -12345).all()


def test_frame_sums_against_the_oracle():
    e = _engine("v2")
    worst = 0.0
    for (n, kind), x in _signals().items():
        want = O.frame_sums(x)
        got = e.debug_join_frames(x).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == want.shape == ((n + 319) // 320,), (n, kind)
        nz = want > 0
        assert not got[~nz].any(), (n, kind)
        err = float(np.max(np.abs(got[nz] - want[nz]) / want[nz])) if nz.any() else 0.0
        worst = max(worst, err)
        assert err <= 1e-12, (n, kind, err)
    print(f"frame sums: worst relative error {worst:.2e} (bound 1e-12)")


def test_frame_sums_do_not_depend_on_the_base():
    import torch
    e = _engine("v2")
    x = _signals()[40000, "from0"] + _signals()[40000, "click"]
    alone = e.debug_join_frames(x).cpu().numpy()
    buf = torch.from_numpy(np.concatenate([np.ones(3, np.float32), x])).to(e.dev)
    assert np.array_equal(e.debug_join_frames(buf[3:]).cpu().numpy(), alone)


def test_span_records_are_the_oracles_integers():
    e = _engine("v2")
    seen = set()
    for (n, kind), x in _signals().items():
        assert O.margin(x, TRIM) > 1e-6, (n, kind)                    # on the oracle alone
        for rate, pause in ((32000, 0.0), (44100, 0.3)):
            want = O.record(x, rate, pause, TRIM)
            buf, span, _ = _join_guarded(e, x, rate, 0, pause, TRIM)
            assert span == want, (n, kind, rate, span, want)
            assert _untouched(buf[want[3]:], 0), (n, kind, rate)
        seen.add((kind, want[0] > 0, want[1] < n))
        # without a trim the span is [0, n)
        assert _join_guarded(e, x, 16000, 1, 0.25)[1] == O.record(x, 16000, 0.25)
    assert {k for k, *_ in seen} == {"silent", "from0", "to_end", "partial_last", "single_frame", "click",
                                     "noise+1dB", "noise-1dB"}
    assert ("click", True, True) in seen and ("from0", False, True) in seen and ("to_end", True, False) in seen
    big = _signals()[40000, "noise+1dB"]
    assert O.record(big, 32000, 0, TRIM)[:2] == (0, 40000) and O.record(_signals()[40000, "noise-1dB"], 32000, 0,
                                                                     TRIM)[:2] == (0, 0)


OUTPUT_CASES = ((0, "silent"), (6400, "silent"), (321, "to_end"), (959, "partial_last"), (6400, "from0"),
                (6400, "single_frame"), (40000, "click"))


@pytest.mark.parametrize("rate", O.RATES)
@pytest.mark.parametrize("fmt", [0, 1])
def test_output_is_the_spans_conversion_then_zeros(rate, fmt):
    e = _engine("v2")
    for n, kind in OUTPUT_CASES:
        x = _signals()[n, kind]
        for pause, trim in ((0.3, TRIM), (0.0, TRIM), (0.01, None)):
            b, en, n_speech, n_out = want = O.record(x, rate, pause, trim)
            buf, span, _ = _join_guarded(e, x, rate, fmt, pause, trim or 0.0)
            assert span == want, (n, kind, rate, pause, trim)
            ref = e.audio_convert(x[b:en], rate, pcm16=bool(fmt)).cpu().numpy()
            assert ref.shape == (n_speech,)
            assert buf[:n_speech].tobytes() == ref.tobytes(), (n, kind, rate, fmt, pause, trim)
            assert buf[n_speech:n_out].tobytes() == bytes(n_out - n_speech) * (4 if fmt == 0 else 2)   # +0.0f / 0
            assert _untouched(buf[n_out:], fmt), (n, kind, rate, fmt)
            got = e.audio_convert(x, rate, pcm16=bool(fmt), pause=pause, trim=trim)            # the Python binding
            assert got.cpu().numpy().tobytes() == buf[:n_out].tobytes()
            if trim is not None:
                assert tuple(e.vits_spans[0].cpu().tolist()) == want


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_loudness_stays_the_untrimmed_items(rate):
    e = _engine("v2")
    n = 40000
    x = np.zeros(n, np.float32)
    x[9000:31000] = (0.2 * np.random.default_rng(5).uniform(-1, 1, 22000)).astype(np.float32)
    assert O.margin(x, TRIM) > 1e-6
    b, en, n_speech, n_out = want = O.record(x, rate, 0.3, TRIM)
    assert (b, en) == (320 * 28 - 640, 320 * 97 + 640)
    whole = e.audio_convert(x, rate, loudness=-16.0)
    stats0 = e.vits_loudness[0].cpu().numpy()
    assert stats0[3] > 0 and stats0[2] != 1.0
    conv = e.audio_convert(x[b:en], rate).cpu().numpy()
    scaled = conv * np.float32(stats0[2])                            # one rounded float32 multiply
    for fmt in (0, 1):
        buf, span, stats = _join_guarded(e, x, rate, fmt, 0.3, TRIM, target=-16.0)
        assert span == want and stats.tobytes() == stats0.tobytes()
        if fmt == 0:
            assert buf[:n_speech].tobytes() == scaled.tobytes()
        else:
            v = np.minimum(np.maximum(scaled * np.float32(32767.0), np.float32(-32768.0)), np.float32(32767.0))
            assert np.array_equal(buf[:n_speech], np.trunc(v).astype(np.int16))
        assert not buf[n_speech:n_out].any() and _untouched(buf[n_out:], fmt)
        got = e.audio_convert(x, rate, pcm16=bool(fmt), loudness=-16.0, pause=0.3, trim=TRIM)
        assert got.cpu().numpy().tobytes() == buf[:n_out].tobytes()
        assert e.vits_loudness[0].cpu().numpy().tobytes() == stats0.tobytes()
    assert whole.shape[0] == O.audio_samples(n, rate)


def test_bad_values_are_refused_before_any_launch():
    import torch
    from genie_tts_amd.engine import Join, _stream, lib
    e = _engine("v2")
    x = torch.zeros(640, device=e.dev)
    out = torch.full((200000,), 7.0, device=e.dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for trim, pause in ((-81.0, 0.0), (-19.0, 0.0), (5.0, 0.0), (float("nan"), 0.0), (0.0, -0.1), (0.0, 5.5),
                        (-50.0, float("nan"))):
        j = Join(0.0, 0.0, None, trim, pause, None)
        assert lib().gsv_audio_join(e.h, p(x), 640, ctypes.byref(j), 32000, 0, p(out), _stream()) == -1
    txt, sem = _utt(8, 10)
    vc = e._vocoder_call([dict(text_seq=txt, pred_semantic=sem, pause=0.3, **_cond("v2"))])   # (keeps the item's tensors)
    item, res = vc.items[0], vc.outs[0]
    assert (vc.specs[0].pause, vc.specs[0].trim) == (np.float32(0.3), 0.0) and res.shape == (640 * 16 + 9600,)
    for j in (Join(0.0, 0.0, None, -10.0, 0.0, None), Join(0.0, 0.0, None, 0.0, 9.0, None)):
        for call in (lambda: lib().gsv_vits_decode_item_join(e.h, ctypes.byref(item), ctypes.byref(j),
                                                             ctypes.c_float(0.5), _stream()),
                     lambda: lib().gsv_vits_decode_batch_join(e.h, 1, ctypes.byref(item), ctypes.byref(j),
                                                              ctypes.c_float(0.5), _stream())):
            assert call() == -1
    item.out = None                                                  # a pause needs `out`
    j = Join(0.0, 0.0, None, 0.0, 0.3, None)
    assert lib().gsv_vits_decode_item_join(e.h, ctypes.byref(item), ctypes.byref(j), ctypes.c_float(0.5),
                                           _stream()) == -1
    assert float(out.min()) == 7.0
    for kw in (dict(pause=6), dict(trim=-10), dict(trim=True)):
        with pytest.raises(ValueError):
            e.vits_decode(txt, sem, **kw, **_cond("v2"))
        with pytest.raises(ValueError):
            e.audio_convert(x, 32000, **kw)


# ------------------------------------------------------------------ through the vocoder
def _items(ver):
    kw = _cond(ver)
    out = []
    for G, S in ((8, 10), (20, 9)):
        txt, sem = _utt(G, S, f"trim{G}")
        out.append(dict(text_seq=txt, pred_semantic=sem, noise_seed=100 + G, **kw))
    return out


def _stage_alone(e, a32, opts):
    """What the stage alone gives for this item's 32 kHz audio and options (spans checked)."""
    x = a32.cpu().numpy()
    rate, pcm = opts.get("sample_rate", 32000), bool(opts.get("pcm16"))
    pause, trim = opts.get("pause", 0.0), opts.get("trim")
    buf, span, _ = _join_guarded(e, x, rate, int(pcm), pause, trim or 0.0)
    if trim is not None:
        assert O.margin(x, trim) > 1e-6
    assert span == O.record(x, rate, pause, trim)
    return buf[:span[3]], span


OPTS = (dict(pause=0.3, trim=-30.0), dict(pause=0.1, trim=-20.0, sample_rate=48000, pcm16=True),
        dict(trim=-40.0, sample_rate=8000), dict(pause=0.25, sample_rate=22050))


def _strip(item):
    return {k: v for k, v in item.items() if k not in ("pause", "trim", "sample_rate", "pcm16")}


def _run(e, how, items):
    """(results cut to their joined lengths, the 32 kHz tensors) of items through one entry point."""
    if how == "item":                                                # (a noise_seed: the batch entry of one)
        it = items[0]
        outs = [e.vits_decode(it["text_seq"], it["pred_semantic"],
                              **{k: v for k, v in it.items() if k not in ("text_seq", "pred_semantic")})]
    elif how == "batch":
        outs = e.vits_decode_batch(items)
    elif how == "batch-async":
        outs = e.vits_decode_batch_async(items)
        e.vits_batch_wait()
        outs = e.vits_joined(outs)
    else:
        outs = [e.vits_decode_async(items[0])]
        e.vits_wait()
        outs = e.vits_joined(outs)
    return outs, list(e.vits_audio_32k)


def test_every_entry_point_gives_the_same_bits(setup):
    """Through every entry point the result is the stage alone on that call's own 32 kHz audio
    (whose spans are the oracle's), and that audio is the one of the same call without options."""
    ver, e = setup
    cases = [(dict(it, **opts), opts) for it in _items(ver) for opts in OPTS]
    for how in ("item", "batch", "batch-async", "async"):
        if how == "async":
            e.set_vocoder_cus(64)
        try:
            for item, opts in cases:
                items = [item, item] if how == "batch-async" else [item]
                bare, _ = _run(e, how, [_strip(it) for it in items])
                bare = [b.cpu().numpy() for b in bare]
                outs, a32 = _run(e, how, items)
                spans = list(e.vits_spans)
                for i in range(len(items)):
                    assert np.array_equal(a32[i].cpu().numpy(), bare[i]), (ver, how, opts)   # untrimmed, bit-unchanged
                    want, span = _stage_alone(e, a32[i], opts)
                    assert outs[i].cpu().numpy().tobytes() == want.tobytes(), (ver, how, opts, i)
                    if "trim" in opts:
                        assert tuple(spans[i].cpu().tolist()) == span
        finally:
            if how == "async":
                e.set_vocoder_cus(0)


def test_the_item_entry_with_eps(setup):
    """gsv_vits_decode_item_join itself (vits_decode reaches it without a noise_seed)."""
    ver, e = setup
    it = _items(ver)[0]
    eps = synth.rng_for("trim-eps").standard_normal((1, 192, 16)).astype(np.float32)
    kw = {k: v for k, v in it.items() if k not in ("text_seq", "pred_semantic", "noise_seed")}
    base = e.vits_decode(it["text_seq"], it["pred_semantic"], eps=eps, **kw).cpu().numpy()
    for opts in OPTS[:2]:
        out = e.vits_decode(it["text_seq"], it["pred_semantic"], eps=eps, **opts, **kw)
        assert np.array_equal(e.vits_audio_32k[0].cpu().numpy(), base)
        want, span = _stage_alone(e, e.vits_audio_32k[0], opts)
        assert out.cpu().numpy().tobytes() == want.tobytes() and tuple(e.vits_spans[0].cpu().tolist()) == span


def test_a_batch_mixes_items_with_both_one_and_no_option(setup):
    ver, e = setup
    a, b = _items(ver)
    opts = [dict(pause=0.3, trim=-30.0, sample_rate=16000), dict(pause=0.2), dict(trim=-20.0, pcm16=True),
            dict(sample_rate=44100), {}]
    items = [dict(it, **o) for it, o in zip((a, b, a, b, a), opts)]
    bare = [x.cpu().numpy() for x in e.vits_decode_batch([_strip(it) for it in items])]
    for run in ("batch", "batch-async"):
        outs, a32 = _run(e, run, items)
        assert [s is not None for s in e.vits_spans] == [True, False, True, False, False]
        for i, o in enumerate(opts):
            assert np.array_equal(a32[i].cpu().numpy(), bare[i]), (ver, run, i)
            if o.keys() & {"pause", "trim"}:
                want, _ = _stage_alone(e, a32[i], o)
            else:
                want = e.audio_convert(a32[i], o.get("sample_rate", 32000)).cpu().numpy()
            assert outs[i].cpu().numpy().tobytes() == want.tobytes(), (ver, run, i)


def test_the_plain_call_is_the_plain_entrys_bits(setup):
    """Without the options each method gives what the plain C entry gives."""
    import torch
    from genie_tts_amd.engine import _check, _stream, lib
    ver, e = setup
    it = _items(ver)[1]
    item, keep, audio = e._vits_item(it)
    _check(lib().gsv_vits_decode_item(e.h, ctypes.byref(item), ctypes.c_float(0.5), _stream()), "plain")
    want = audio.cpu().numpy().copy()
    assert np.array_equal(e.vits_decode_batch([it])[0].cpu().numpy(), want)
    assert np.array_equal(e.vits_decode_batch([dict(it, pause=0, trim=None)])[0].cpu().numpy(), want)
    outs = e.vits_decode_batch_async([it])
    e.vits_batch_wait()
    assert np.array_equal(e.vits_joined(outs)[0].cpu().numpy(), want) and e.vits_spans == [None]
    e.set_vocoder_cus(64)
    try:
        out = e.vits_decode_async(it)
        e.vits_wait()
    finally:
        e.set_vocoder_cus(0)
    assert np.array_equal(out.cpu().numpy(), want)
    x = torch.from_numpy(want).to(e.dev)
    conv = e.audio_convert(x, 24000, pcm16=True).cpu().numpy()
    item, keep, out = e._vits_item(dict(it, sample_rate=24000, pcm16=True))
    _check(lib().gsv_vits_decode_item(e.h, ctypes.byref(item), ctypes.c_float(0.5), _stream()), "plain")
    assert np.array_equal(out.cpu().numpy(), conv)
    assert np.array_equal(e.vits_decode_batch([dict(it, sample_rate=24000, pcm16=True)])[0].cpu().numpy(), conv)


def test_fp16_range_rerun_measures_the_reruns_audio(setup):
    """test_vits_gpu.py's recipe (eps x 1e6): the span and `out` are those of the re-run's audio."""
    ver, e = setup
    it = _items(ver)[0]
    eps = (synth.rng_for("trim-big").standard_normal((1, 192, 16)) * 1e6).astype(np.float32)
    kw = {k: v for k, v in it.items() if k not in ("text_seq", "pred_semantic", "noise_seed")}
    opts = dict(pause=0.1, trim=-20.0, sample_rate=16000)
    n0 = e.counter("vits_f32_reruns")
    out = e.vits_decode(it["text_seq"], it["pred_semantic"], eps=eps, **opts, **kw)
    assert e.counter("vits_f32_reruns") == n0 + 1
    want, _ = _stage_alone(e, e.vits_audio_32k[0], opts)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    e.set_vocoder_cus(64)
    try:
        out = e.vits_decode_async(dict(it, noise_seed=None, eps=eps, **opts))
        e.vits_wait()
        out = e.vits_joined([out])[0]
    finally:
        e.set_vocoder_cus(0)
    assert e.counter("vits_f32_reruns") == n0 + 2
    assert out.cpu().numpy().tobytes() == want.tobytes()
