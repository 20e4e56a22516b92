"""CPU: the sentence join's options (engine.vocoder_options, `pause` and `trim`), the exported
pause length where float32 and double disagree, the gsv_join layout, and the float64 oracle
(tests/trim_oracle.py) on hand-built signals whose spans are known."""
import ctypes

import numpy as np
import pytest

from genie_tts_amd import engine as E
from genie_tts_amd.engine import check_join, vocoder_options, vocoder_options_each
from tests import trim_oracle as O


def test_options_are_named_and_validated_with_the_other_five():
    assert E.VOCODER_OPTIONS == ("speed", "sample_rate", "pcm16", "loudness", "peak", "pause", "trim")
    assert vocoder_options() == {} and vocoder_options(pause=None, trim=None) == {}
    assert vocoder_options(pause=0) == {} and vocoder_options(pause=0.0) == {}       # 0: none, today's call
    assert vocoder_options(pause=0.3) == dict(pause=0.3) and vocoder_options(trim=-50) == dict(trim=-50.0)
    assert vocoder_options(pause=5, trim=-80) == dict(pause=5.0, trim=-80.0)
    assert vocoder_options(pause=np.float32(0.5), trim=np.int64(-20)) == dict(pause=0.5, trim=-20.0)
    assert vocoder_options(1.0, None, False, None, None, 0.3, -50) == dict(pause=0.3, trim=-50.0)   # appended
    assert vocoder_options(1.1, 8000, True, -16, 0.5, 0.3, -50) == dict(
        speed=1.1, sample_rate=8000, pcm16=True, loudness=-16.0, peak=0.5, pause=0.3, trim=-50.0)
    assert check_join() == {} and check_join(0.3, -50) == dict(pause=0.3, trim=-50.0)
    for bad in (-0.001, 5.001, True, False, float("nan"), float("inf"), "0.3", [0.3], np.bool_(True)):
        with pytest.raises(ValueError, match="pause"):
            vocoder_options(pause=bad)
        with pytest.raises(ValueError, match="pause"):
            vocoder_options(speed=1.1, sample_rate=8000, loudness=-16, pause=bad, trim=-50)
    for bad in (-80.5, -19.9, 0, 0.0, 10, True, False, float("nan"), float("-inf"), "-50", (-50,)):
        with pytest.raises(ValueError, match="trim"):
            vocoder_options(trim=bad)
        with pytest.raises(ValueError, match="trim"):
            check_join(0.3, bad)


def test_one_value_or_one_per_item():
    assert vocoder_options_each(3, pause=0.3, trim=-50) == [dict(pause=0.3, trim=-50.0)] * 3
    assert vocoder_options_each(3, pause=[0.3, None, 0], trim=[None, -40, None]) == [
        dict(pause=0.3), dict(trim=-40.0), {}]
    assert vocoder_options_each(2, 1.0, None, False, None, None, [0.1, 0.2], -30) == [
        dict(pause=0.1, trim=-30.0), dict(pause=0.2, trim=-30.0)]
    assert vocoder_options_each(2, loudness=[-16, None], pause=0.5) == [dict(loudness=-16.0, pause=0.5),
                                                                       dict(pause=0.5)]
    for name, v in (("pause", [0.3, 0.3]), ("trim", [-50] * 4)):
        with pytest.raises(ValueError, match="pause / trim: one value, or one per item"):
            vocoder_options_each(3, **{name: v})
    with pytest.raises(ValueError, match="trim"):
        vocoder_options_each(3, trim=[-50, -10, -50])
    with pytest.raises(ValueError, match="pause"):
        vocoder_options_each(2, pause=[0.1, True])


def test_the_join_struct_is_the_headers():
    names = [n for n, _ in E.Join._fields_]
    assert names == ["target", "peak", "stats", "trim", "pause", "span"]
    assert ctypes.sizeof(E.Join) == 32
    assert [getattr(E.Join, n).offset for n in names] == [0, 4, 8, 16, 20, 24]
    assert names[:3] == [n for n, _ in E.Loudness._fields_]          # it carries the loudness fields
    z = E.Join()
    assert (z.target, z.peak, z.stats, z.trim, z.pause, z.span) == (0.0, 0.0, None, 0.0, 0.0, None)
    assert (E.JOIN_FRAME, E.JOIN_GUARD) == (O.FRAME, O.GUARD) == (320, 640)


def test_pause_samples_where_float32_and_double_disagree():
    """pause_n = (int)((double)rate * (double)(float32)pause): a caller who multiplies the Python
    float gets another count at some values, so the count comes from the library alone."""
    pairs = []
    for rate in O.RATES:
        for k in range(1, 5001):
            p = k / 1000.0
            f32, f64 = int(float(rate) * float(np.float32(p))), int(float(rate) * p)
            if f32 != f64:
                pairs.append((rate, p, f32, f64))
    assert pairs, "no pause at which float32 and double disagree"
    print(f"{len(pairs)} (rate, pause) pairs disagree, the first {pairs[0]}")
    assert {r for r, *_ in pairs} == set(O.RATES)                     # at every rate
    for rate, p, f32, f64 in pairs[:200]:
        assert E.join_pause_samples(rate, p) == f32 == O.pause_samples(rate, p) != f64
    for rate in O.RATES:
        for p in (0.0, 0.3, 1.0, 2.5, 5.0):
            assert E.join_pause_samples(rate, p) == O.pause_samples(rate, p)
            for n in (0, 1, 321, 40000):
                assert E.join_samples(n, rate, p) == O.audio_samples(n, rate) + O.pause_samples(rate, p)
                assert E.audio_samples(n, rate) == O.audio_samples(n, rate)
    assert E.lib().gsv_join_pause_samples(0, ctypes.c_float(0.5)) == 16000            # rate 0 means 32000
    for rate, p in ((12345, 0.3), (32000, -0.1), (32000, 5.5), (32000, float("nan"))):
        assert E.lib().gsv_join_pause_samples(rate, ctypes.c_float(p)) == -1
        assert E.lib().gsv_join_samples(100, rate, ctypes.c_float(p)) == -1
    with pytest.raises(ValueError):
        E.join_pause_samples(32000, 6)
    with pytest.raises(ValueError):
        E.join_samples(10, 11025, 0.3)


def _tone(n, amp):
    return (amp * np.sin(0.05 * np.arange(n))).astype(np.float32)


def test_oracle_on_signals_with_known_spans():
    T = O.threshold(-50)
    assert abs(T - 1e-5) < 1e-18 and O.threshold(-20) == 10.0 ** -2.0
    x = np.zeros(6400, np.float32)
    assert O.span(x, -50) == (0, 0) and O.record(x, 32000, 0.3, -50) == (0, 0, 0, 9600)
    assert O.span(x) == (0, 6400) and O.record(x, 48000, 0.3) == (0, 6400, 9600, 9600 + 14400)
    x[1600:3200] = _tone(1600, 0.5)                                  # frames 5 .. 9
    assert list(np.flatnonzero(O.active(x, -50))) == [5, 6, 7, 8, 9]
    assert O.span(x, -50) == (1600 - 640, 3200 + 640)
    assert O.record(x, 16000, 1.0, -50) == (960, 3840, 1440, 1440 + 16000)
    assert O.join(x, 0.01, -50).shape == (2880 + 319,) and not O.join(x, 0.01, -50)[2880:].any()   # float32 0.01 < 0.01
    assert np.array_equal(O.join(x, None, -50), x[960:3840]) and np.array_equal(O.join(x), x)
    y = np.zeros(6400, np.float32)
    y[:400] = 0.5                                                    # from sample 0: the guard clips at 0
    assert O.span(y, -50) == (0, 640 + 640)
    y = np.zeros(6400, np.float32)
    y[6000:] = 0.5                                                   # to the last sample: clipped at n
    assert O.span(y, -50) == (320 * 18 - 640, 6400)
    y = np.zeros(961, np.float32)
    y[960] = 0.5                                                     # only the partial last frame (c = 1)
    assert list(O.frame_counts(961)) == [320, 320, 320, 1] and O.span(y, -50) == (320, 961)
    y[960] = 0.001                                                   # 1e-6 < T * 1: silent
    assert O.span(y, -50) == (0, 0)
    y = np.zeros(40000, np.float32)
    y[20000] = 0.9                                                   # a click: one active frame
    assert O.span(y, -50) == (320 * 62 - 640, 320 * 63 + 640) and O.margin(y, -50) > 1e-6
    assert O.span(np.zeros(0, np.float32), -50) == (0, 0) and O.margin(np.zeros(0, np.float32), -50) == np.inf
    s = O.frame_sums(np.full(321, 0.5, np.float32))
    assert list(s) == [80.0, 0.25]
