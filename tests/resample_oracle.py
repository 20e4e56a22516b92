"""The float64 numpy statement of the engine's output stage (include/genie_engine.h, the
"Output format" paragraph of gsv_vits_item): the polyphase resample from 32 kHz with
scipy.signal.resample_poly's default filter -- restated, no scipy in it -- and the int16 rule.
The GPU tests compare the engine against it; tests/test_sample_rate_host.py compares it against
scipy."""
from math import gcd

import numpy as np

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
BAD_RATES = (-8000, 1, 11025, 12000, 12345, 32001, 96000)


def ratio(out_rate: int):
    g = gcd(32000, out_rate)
    return out_rate // g, 32000 // g


def n_out(n_in: int, out_rate: int) -> int:
    up, down = ratio(out_rate)
    return -(-n_in * up // down)


def bessel_i0(x: float) -> float:
    """I0 from its power series, in double."""
    s = t = 1.0
    k = 1
    while True:
        t *= (x / 2.0) ** 2 / (k * k)
        s += t
        k += 1
        if t < s * 1e-17:
            return s


def taps(out_rate: int):
    """(h float64 [2 half + 1], half): Kaiser(5) windowed sinc, sum 1, times up."""
    up, down = ratio(out_rate)
    m = max(up, down)
    half = 10 * m
    n = np.arange(2 * half + 1) - half
    w = np.array([bessel_i0(5.0 * np.sqrt(max(0.0, 1.0 - (k / half) ** 2))) for k in n]) / bessel_i0(5.0)
    t = n / m
    sinc = np.where(n == 0, 1.0, np.sin(np.pi * t) / np.where(n == 0, 1.0, np.pi * t))
    h = (1.0 / m) * sinc * w
    return h / h.sum() * up, half


_taps = {}


def resample(x, out_rate: int, h=None) -> np.ndarray:
    """y[k] = sum_n h[k down + half - n up] x[n], zeros outside the signal; float64.
    h: other taps of the same length (the float32-rounded ones, for the error bound)."""
    x = np.asarray(x, np.float64).reshape(-1)
    if out_rate == 32000:
        return x.copy()
    up, down = ratio(out_rate)
    if out_rate not in _taps:
        _taps[out_rate] = taps(out_rate)
    h0, half = _taps[out_rate]
    h = h0 if h is None else np.asarray(h, np.float64)
    k = np.arange(n_out(x.size, out_rate), dtype=np.int64)
    c = k * down + half
    hi = c // up                                   # the largest n with h index >= 0
    q = (2 * half) // up + 1                       # taps a phase can hold
    n = hi[:, None] - np.arange(q)[None, :]        # [n_out][q]
    j = c[:, None] - n * up                        # h index, >= 0
    ok = (n >= 0) & (n < x.size) & (j <= 2 * half)
    return np.where(ok, h[np.minimum(j, 2 * half)] * x[np.clip(n, 0, max(x.size - 1, 0))], 0.0).sum(axis=1) \
        if x.size else np.zeros(0)


def pcm16(y) -> np.ndarray:
    """(int16) trunc(min(max(y * 32767, -32768), 32767)): the reference's (x * 32767).astype(int16)
    with saturation."""
    return np.trunc(np.clip(np.asarray(y, np.float64) * 32767.0, -32768.0, 32767.0)).astype(np.int16)


def abs_h_phase_sum(out_rate: int) -> float:
    """max over the phases of sum |h|: the factor of the float32 chain's error bound."""
    up, _ = ratio(out_rate)
    h, _ = taps(out_rate) if out_rate not in _taps else _taps[out_rate]
    return max(float(np.abs(h[p::up]).sum()) for p in range(up))
