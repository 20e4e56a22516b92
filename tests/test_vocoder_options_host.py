"""CPU: engine.vocoder_options / vocoder_options_each, the one place a vocoder call's five options
(speed, sample_rate, pcm16, loudness, peak) are validated and reduced to the keys that differ from
the call without them, and the Engine's four vocoder methods and audio_convert reaching the `_join` C
entries with NULL or a filled gsv_join array, over a recording stand-in for the library."""
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
    """Stands in for lib(): every gsv_* call is recorded and succeeds; gsv_vits_frames,
    gsv_audio_samples and gsv_join_samples are the real ones."""

    def __init__(self):
        self.calls = []
        self.hook = None                                              # called with (name, args) of each recorded call
        self.real = E.lib()

    def __getattr__(self, name):
        if name in ("gsv_vits_frames", "gsv_audio_samples", "gsv_join_samples"):
            return getattr(self.real, name)
        def call(*a):
            self.calls.append((name, a))
            if self.hook:
                self.hook(name, a)
            return 0
        return call


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


def _plain(j):
    """This gsv_join entry carries no join option."""
    return j.trim == 0.0 and j.pause == 0.0 and not j.span


CALLS = (("gsv_vits_decode_item_join", 2, lambda e, it: e.vits_decode(it["text_seq"], it["pred_semantic"],
                                                                        **{k: v for k, v in it.items()
                                                                           if k not in ("text_seq", "pred_semantic")})),
         ("gsv_vits_decode_batch_join", 3, lambda e, it: e.vits_decode(it["text_seq"], it["pred_semantic"], noise_seed=7,
                                                                         **{k: v for k, v in it.items()
                                                                            if k not in ("text_seq", "pred_semantic")})),
         ("gsv_vits_decode_batch_join", 3, lambda e, it: e.vits_decode_batch([it])[0]),
         ("gsv_vits_decode_batch_async_join", 3, lambda e, it: e.vits_decode_batch_async([it])[0]),
         ("gsv_vits_decode_async_join", 2, lambda e, it: e.vits_decode_async(it)))


def test_the_four_methods_always_reach_the_norm_entries(stub):
    # (the name is from when the methods reached the `_norm` entries; they reach the `_join` ones, which
    # those forward to, and this test pins that)
    e, L = stub
    for name, at, run in CALLS:
        for opts in ({}, dict(speed=1.1), dict(sample_rate=16000, pcm16=True), dict(peak=0.5)):
            L.calls.clear()
            out = run(e, _item(**opts))
            assert [c[0] for c in L.calls] == [name], (name, opts)
            assert L.calls[0][1][at] is None                          # no target: NULL, the plain call
            assert e.vits_loudness == [None] and e.vits_spans == [None]
            frames = E.vits_frames(8, opts.get("speed", 1.0))
            assert out.shape == (E.audio_samples(640 * frames, opts.get("sample_rate", 32000)),)
            assert out.dtype == (e.torch.int16 if opts.get("pcm16") else e.torch.float32)
        for opts, peak in ((dict(loudness=-16), 0.0), (dict(loudness=-23.5, peak=0.5, sample_rate=8000), 0.5)):
            L.calls.clear()
            out = run(e, _item(**opts))
            assert [c[0] for c in L.calls] == [name], (name, opts)
            spec = L.calls[0][1][at]
            assert len(spec) == 1 and isinstance(spec[0], E.Join)
            ld = spec[0]
            assert (ld.target, ld.peak) == (opts["loudness"], peak) and _plain(ld)
            stats = e.vits_loudness[0]
            assert stats.shape == (4,) and stats.dtype == e.torch.float32 and ld.stats == stats.data_ptr()
            assert out.shape == (E.audio_samples(1280 * 8, opts.get("sample_rate", 32000)),)
            assert e.vits_audio_32k[0].shape == (1280 * 8,) and e.vits_audio_32k[0] is not out


def test_a_pause_and_a_trim_reach_the_join_entries(stub):
    """pause: the float32 value, no span record, the result of the joined length; trim: the span
    record is a row of the call's one int32 [k, 4] tensor."""
    e, L = stub
    for name, at, run in CALLS:
        L.calls.clear()
        out = run(e, _item(pause=0.3, sample_rate=16000))
        assert [c[0] for c in L.calls] == [name]
        j, = L.calls[0][1][at]
        assert j.pause == np.float32(0.3) and j.trim == 0.0 and not j.span and (j.target, j.peak, j.stats) == (0, 0, None)
        assert out.shape == (E.join_samples(1280 * 8, 16000, 0.3),) == (5120 + 4800,)
        assert e.vits_spans == [None] and e.vits_loudness == [None] and e.vits_audio_32k[0].shape == (1280 * 8,)
    # (a trim is read back by vits_joined: the batch-async method returns before that)
    L.calls.clear()
    outs = e.vits_decode_batch_async([_item(trim=-50)])
    (name, args), = L.calls
    j, = args[3]
    assert name == "gsv_vits_decode_batch_async_join" and j.trim == -50.0 and j.pause == 0.0 and not j.stats
    sp, = e.vits_spans
    assert sp.shape == (4,) and sp.dtype == e.torch.int32 and j.span == sp.data_ptr()
    assert sp._base is e._vits_call.span_all and e._vits_call.span_all.shape == (1, 4)
    assert outs[0].shape == (E.join_samples(1280 * 8, 32000, 0.0),) == (1280 * 8,)
    e._vits_call.span_all[0, 3] = 777                                 # (what the stage would write)
    assert e.vits_joined(outs)[0].shape == (777,)


def test_only_the_middle_item_of_a_batch_trims(stub):
    e, L = stub
    outs = e.vits_decode_batch_async([_item(), _item(trim=-30, pause=0.1), _item(sample_rate=8000)])
    (name, args), = L.calls
    assert name == "gsv_vits_decode_batch_async_join" and args[1] == 3 and len(args[3]) == 3
    assert _plain(args[3][0]) and _plain(args[3][2])
    assert (args[3][1].trim, args[3][1].pause) == (-30.0, np.float32(0.1))
    assert [s is not None for s in e.vits_spans] == [False, True, False]
    assert args[3][1].span == e.vits_spans[1].data_ptr() and e._vits_call.span_all.shape == (1, 4)
    e._vits_call.span_all[0, 3] = 55
    assert [o.shape[0] for o in e.vits_joined(outs)] == [1280 * 8, 55, 2560]


def test_audio_convert_is_one_join_call(stub):
    e, L = stub
    x = np.zeros(6400, np.float32)
    e.vits_decode_batch([_item(loudness=-16)])
    last = (e.vits_audio_32k, e.vits_loudness, e.vits_spans)
    # the stand-in's stage writes n_out = 777 into the span record it is given
    L.hook = lambda name, a: a[3] is not None and a[3][0].span and \
        (ctypes.c_int32 * 4).from_address(a[3][0].span).__setitem__(3, 777)
    for opts in ({}, dict(loudness=-16.0, peak=0.5), dict(pause=0.25, trim=-40)):
        L.calls.clear()
        out = e.audio_convert(x, 48000, pcm16=True, **opts)
        (name, args), = L.calls
        assert name == "gsv_audio_join" and args[2] == 6400 and args[4:6] == (48000, 1)
        assert out.dtype == e.torch.int16
        if not opts:
            assert args[3] is None and out.shape == (9600,)
            assert (e.vits_audio_32k, e.vits_loudness, e.vits_spans) == last   # the plain conversion is no call
            continue
        j, = args[3]
        assert (j.target, j.peak, j.trim, j.pause) == (opts.get("loudness", 0.0), opts.get("peak", 0.0),
                                                       opts.get("trim", 0.0), opts.get("pause", 0.0))
        assert (e.vits_loudness[0] is not None) == ("loudness" in opts) == bool(j.stats)
        assert (e.vits_spans[0] is not None) == ("trim" in opts) == bool(j.span)
        assert e.vits_audio_32k is last[0]                            # stays the last vocoder call's
        if "trim" in opts:
            assert j.span == e.vits_spans[0].data_ptr() and e.vits_spans[0].dtype == e.torch.int32
            assert E.join_samples(6400, 48000, 0.25) == 9600 + 12000 and out.shape == (777,)   # the buffer, cut to n_out
        else:
            assert j.stats == e.vits_loudness[0].data_ptr() and out.shape == (9600,)
            assert e.vits_spans is last[2] and e._vits_call.a32 is last[0]   # a target alone leaves the last call's spans
    with pytest.raises(ValueError):
        e.audio_convert(x, 48000, trim=-10)
    assert len(L.calls) == 1                                          # refused before any call


def test_a_batch_mixes_items_with_and_without_a_target(stub):
    e, L = stub
    e.vits_decode_batch([_item(), _item(loudness=-16, peak=1), _item(sample_rate=8000)])
    (name, args), = L.calls
    assert name == "gsv_vits_decode_batch_join" and args[1] == 3
    assert [(l.target, l.peak, bool(l.stats)) for l in args[3]] == [(0.0, 0.0, False), (-16.0, 1.0, True),
                                                                    (0.0, 0.0, False)]
    assert all(isinstance(l, E.Join) and _plain(l) for l in args[3])
    assert [s is not None for s in e.vits_loudness] == [False, True, False]
    with pytest.raises(ValueError):
        e.vits_decode_batch([_item(), _item(loudness=-4)])
    with pytest.raises(ValueError):
        e.vits_decode(np.arange(3), np.arange(8), speed=9.0)
    assert len(L.calls) == 1                                          # refused before any call
