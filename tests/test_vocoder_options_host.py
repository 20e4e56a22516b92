"""CPU: engine.vocoder_options / vocoder_options_each, the one place a vocoder call's five options
(speed, sample_rate, pcm16, loudness, peak) are validated and reduced to the keys that differ from
the call without them, and the Engine's four vocoder methods reaching the `_norm` C entries with
NULL or a filled gsv_loudness, over a recording stand-in for the library."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from genie_tts_amd import engine as E
from genie_tts_amd.engine import check_loudness, check_out_format, vocoder_options, vocoder_options_each


def test_equals_the_three_parts_over_the_grid():
    n = 0
    for sp, rate, pcm, loud, peak in itertools.product((None, 1, 1.0, 0.25, 1.1, 4), (None, 8000, 32000, 48000),
                                                       (False, True), (None, -50, -16, -5), (None, 0.5, 1)):
        want = {} if sp is None or sp == 1 else {"speed": float(sp)}
        want.update(check_out_format(rate, pcm))
        want.update(check_loudness(loud, peak))
        got = vocoder_options(sp, rate, pcm, loud, peak)
        assert got == want, (sp, rate, pcm, loud, peak)
        assert all(type(got[k]) is float for k in ("speed", "loudness", "peak") if k in got)
        assert got == vocoder_options(speed=sp, sample_rate=rate, pcm16=pcm, loudness=loud, peak=peak)
        n += 1
    assert n == 6 * 4 * 2 * 4 * 3
    assert vocoder_options() == {}
    assert vocoder_options(peak=0.5) == {} and vocoder_options(1.0, None, False, None, 1) == {}


@pytest.mark.parametrize("bad", [dict(speed=0.2), dict(speed=4.5), dict(speed=math.nan), dict(speed="fast"),
                                 dict(sample_rate=12345), dict(sample_rate=16000.5), dict(sample_rate="16000"),
                                 dict(sample_rate=True), dict(loudness=-4), dict(loudness=0), dict(loudness="x"),
                                 dict(loudness=-16, peak=0), dict(loudness=-16, peak=1.5), dict(peak=0),
                                 dict(peak=1.5)], ids=str)
def test_each_single_bad_field_raises(bad):
    with pytest.raises(ValueError):
        vocoder_options(**bad)
    with pytest.raises(ValueError):                                   # ... whatever else is given
        vocoder_options(**dict(dict(speed=1.1, sample_rate=8000, pcm16=True, loudness=-16, peak=0.5), **bad))


def test_messages_are_those_of_the_three_checks():
    for kw, first in ((dict(speed=9), lambda: E.vits_frames(0, 9)), (dict(speed="fast"), lambda: E.vits_frames(0, "fast")),
                      (dict(sample_rate=12345), lambda: check_out_format(12345)),
                      (dict(loudness=-4), lambda: check_loudness(-4)), (dict(peak=2), lambda: check_loudness(None, 2))):
        with pytest.raises(ValueError) as want:
            first()
        with pytest.raises(ValueError) as got:
            vocoder_options(**kw)
        assert str(got.value) == str(want.value)


def test_each_broadcasts_one_value_or_one_per_item():
    kw = dict(speed=1.1, sample_rate=8000, pcm16=True, loudness=-16, peak=0.5)
    assert vocoder_options_each(3, **kw) == [vocoder_options(**kw)] * 3
    assert vocoder_options_each(3) == [{}] * 3 and vocoder_options_each(0) == []
    assert vocoder_options_each(3, np.float32(0.5)) == [dict(speed=0.5)] * 3
    # the lists of test_loudness_host.py's test_tts_batch_vocoder_takes_one_value_or_one_per_item
    assert vocoder_options_each(3, loudness=[-16, None, -23], peak=[None, 0.5, 0.25], sample_rate=[None, 8000, 48000],
                                pcm16=[False, True, True]) == \
        [dict(loudness=-16.0), dict(sample_rate=8000, pcm16=True),
         dict(loudness=-23.0, peak=0.25, sample_rate=48000, pcm16=True)]
    assert vocoder_options_each(2, speed=[1.0, 2], loudness=-16) == [dict(loudness=-16.0), dict(speed=2.0, loudness=-16.0)]
    for name, v, msg in (("speed", [1.0, 1.1], "speed"), ("sample_rate", [8000], "sample_rate / pcm16"),
                         ("pcm16", [True] * 4, "sample_rate / pcm16"), ("loudness", [-16, -16], "loudness / peak"),
                         ("peak", [0.5], "loudness / peak")):
        with pytest.raises(ValueError) as e:
            vocoder_options_each(3, **{name: v})
        assert str(e.value) == f"{msg}: one value, or one per item"
    for bad in (dict(loudness=[-16, -4, -16]), dict(speed=[1.0, 9.0, 1.0]), dict(sample_rate=[None, 12345, None])):
        with pytest.raises(ValueError):                               # one bad item fails the batch
            vocoder_options_each(3, **bad)


# ------------------------------------------------------------------ the Engine over a recording library
class _Lib:
    """Stands in for lib(): every gsv_* call is recorded and succeeds; gsv_vits_frames and
    gsv_audio_samples are the real ones."""

    def __init__(self):
        self.calls = []
        self.real = E.lib()

    def __getattr__(self, name):
        if name in ("gsv_vits_frames", "gsv_audio_samples"):
            return getattr(self.real, name)
        return lambda *a: self.calls.append((name, a)) or 0


@pytest.fixture
def stub(monkeypatch):
    import torch
    L = _Lib()
    monkeypatch.setattr(E, "lib", lambda: L)
    monkeypatch.setattr(E, "_stream", lambda: ctypes.c_void_p(0))
    e = E.Engine.__new__(E.Engine)
    e.torch, e.dev, e.h = torch, torch.device("cpu"), None
    return e, L


def _item(**kw):
    return dict(text_seq=np.arange(3), pred_semantic=np.arange(8), ref_audio=np.zeros(64, np.float32), **kw)


def _loudness_arg(arg):
    """The gsv_loudness a recorded call passed: byref of one, or an array of them."""
    return arg._obj if hasattr(arg, "_obj") else arg[0]


def test_the_four_methods_always_reach_the_norm_entries(stub):
    e, L = stub
    calls = (("gsv_vits_decode_item_norm", 2, lambda it: e.vits_decode(it["text_seq"], it["pred_semantic"],
                                                                         **{k: v for k, v in it.items()
                                                                            if k not in ("text_seq", "pred_semantic")})),
             ("gsv_vits_decode_batch_norm", 3, lambda it: e.vits_decode(it["text_seq"], it["pred_semantic"], noise_seed=7,
                                                                          **{k: v for k, v in it.items()
                                                                             if k not in ("text_seq", "pred_semantic")})),
             ("gsv_vits_decode_batch_norm", 3, lambda it: e.vits_decode_batch([it])[0]),
             ("gsv_vits_decode_batch_async_norm", 3, lambda it: e.vits_decode_batch_async([it])[0]),
             ("gsv_vits_decode_async_norm", 2, lambda it: e.vits_decode_async(it)))
    for name, at, run in calls:
        for opts in ({}, dict(speed=1.1), dict(sample_rate=16000, pcm16=True), dict(peak=0.5)):
            L.calls.clear()
            out = run(_item(**opts))
            assert [c[0] for c in L.calls] == [name], (name, opts)
            assert L.calls[0][1][at] is None                          # no target: NULL, the plain call
            assert e.vits_loudness == [None]
            frames = E.vits_frames(8, opts.get("speed", 1.0))
            assert out.shape == (E.audio_samples(640 * frames, opts.get("sample_rate", 32000)),)
            assert out.dtype == (e.torch.int16 if opts.get("pcm16") else e.torch.float32)
        for opts, peak in ((dict(loudness=-16), 0.0), (dict(loudness=-23.5, peak=0.5, sample_rate=8000), 0.5)):
            L.calls.clear()
            out = run(_item(**opts))
            assert [c[0] for c in L.calls] == [name], (name, opts)
            ld = _loudness_arg(L.calls[0][1][at])
            assert isinstance(ld, E.Loudness) and (ld.target, ld.peak) == (opts["loudness"], peak)
            stats = e.vits_loudness[0]
            assert stats.shape == (4,) and stats.dtype == e.torch.float32 and ld.stats == stats.data_ptr()
            assert out.shape == (E.audio_samples(1280 * 8, opts.get("sample_rate", 32000)),)
            assert e.vits_audio_32k[0].shape == (1280 * 8,) and e.vits_audio_32k[0] is not out


def test_a_batch_mixes_items_with_and_without_a_target(stub):
    e, L = stub
    e.vits_decode_batch([_item(), _item(loudness=-16, peak=1), _item(sample_rate=8000)])
    (name, args), = L.calls
    assert name == "gsv_vits_decode_batch_norm" and args[1] == 3
    assert [(l.target, l.peak, bool(l.stats)) for l in args[3]] == [(0.0, 0.0, False), (-16.0, 1.0, True),
                                                                    (0.0, 0.0, False)]
    assert [s is not None for s in e.vits_loudness] == [False, True, False]
    with pytest.raises(ValueError):
        e.vits_decode_batch([_item(), _item(loudness=-4)])
    with pytest.raises(ValueError):
        e.vits_decode(np.arange(3), np.arange(8), speed=9.0)
    assert len(L.calls) == 1                                          # refused before any call
