"""float64 restatement of the loudness stage (include/genie_engine.h, gsv_loudness): ITU-R
BS.1770-4 K-weighting, 100 ms hop energies, 400 ms blocks at 75 % overlap, the two gates, the
engine's rules for what the standard leaves open, and the gain under a peak ceiling.  numpy and
scipy on the CPU; never imports the engine."""
import math

import numpy as np

HOP = 3200            # 100 ms at 32 kHz
BLOCK = 4 * HOP
ABS_GATE = -70.0
DEFAULT_PEAK = 10.0 ** (-1.0 / 20.0)    # -1 dBFS (EBU R 128)


def coeffs(rate):
    """(b_shelf, a_shelf, b_hp, a_hp), each three float64 values."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return b1, a1, b2, a2


def coeffs10(rate):
    """The layout of gsv_loudness_coeffs: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2."""
    b1, a1, b2, a2 = coeffs(rate)
    return np.concatenate([b1, a1[1:], b2, a2[1:]])


def kweight(x, rate=32000, dtype=np.float64):
    """The K-weighted signal; dtype float32 is the sequential float32 form (coefficients, state
    and samples all float32), the yardstick for the GPU's rounding."""
    from scipy.signal import lfilter
    b1, a1, b2, a2 = (c.astype(dtype) for c in coeffs(rate))
    x = np.asarray(x, dtype)
    if x.size == 0:
        return x
    return lfilter(b2, a2, lfilter(b1, a1, x).astype(dtype)).astype(dtype)


def hops(x, rate=32000, dtype=np.float64, hop=None):
    """e[n // hop]: the energy of each full 100 ms hop of the K-weighted signal."""
    hop = hop or rate // 10
    y = kweight(x, rate, dtype).astype(np.float64)
    m = y.size // hop
    return (y[:m * hop].reshape(m, hop) ** 2).sum(axis=1)


def _lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0 else -math.inf


def measure(x, rate=32000):
    """dict(loudness, peak, blocks_kept, blocks, past_abs, block_lufs, gamma)."""
    x = np.asarray(x, np.float64)
    hop = rate // 10
    n = x.size
    peak = float(np.abs(x).max()) if n else 0.0
    out = dict(loudness=-math.inf, peak=peak, blocks_kept=0, blocks=0, past_abs=0, block_lufs=np.zeros(0),
               gamma=-math.inf)
    if n == 0:
        return out
    if n < 4 * hop:                       # one ungated block over all n samples
        y = kweight(x, rate)
        L = _lufs(float((y ** 2).sum()) / n)
        out.update(loudness=L, blocks_kept=int(L > ABS_GATE), blocks=1, past_abs=int(L > ABS_GATE),
                   block_lufs=np.array([L]))
        return out
    e = hops(x, rate)
    z = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4 * hop)
    l = np.array([_lufs(v) for v in z])
    out.update(blocks=z.size, block_lufs=l)
    a = l > ABS_GATE
    out["past_abs"] = int(a.sum())
    if not a.any():
        return out
    gamma = _lufs(float(z[a].mean())) - 10.0
    k = a & (l > gamma)
    out["gamma"] = gamma
    if k.any():
        out.update(loudness=_lufs(float(z[k].mean())), blocks_kept=int(k.sum()))
    return out


def loudness(x, rate=32000):
    return measure(x, rate)["loudness"]


def gain(loudness_lufs, peak, target, ceiling=None, blocks_kept=1):
    """min(10^((target - loudness) / 20), ceiling / peak); 1 when nothing was kept."""
    if blocks_kept == 0 or not math.isfinite(loudness_lufs):
        return 1.0
    ceiling = DEFAULT_PEAK if not ceiling else ceiling
    g = 10.0 ** ((target - loudness_lufs) / 20.0)
    return min(g, ceiling / peak) if peak > 0 else g


def gate_margin(x, rate=32000):
    """The least distance (LU) of any block from the absolute gate and from the relative gate."""
    m = measure(x, rate)
    l = m["block_lufs"]
    l = l[np.isfinite(l)]
    if l.size == 0:
        return math.inf
    d = np.abs(l - ABS_GATE).min()
    if math.isfinite(m["gamma"]) and m["blocks"] > 1:
        d = min(d, np.abs(l[l > ABS_GATE] - m["gamma"]).min())
    return float(d)


def signals():
    """The four test signals of the loudness tests, float32 at 32 kHz: each from its own
    default_rng(2024), its segments drawn in order as a * uniform(-1, 1, m)."""
    def draw(*segs):
        r = np.random.default_rng(2024)
        return np.concatenate([a * r.uniform(-1, 1, m) for a, m in segs])
    steady = draw((0.3, 32000))
    speech = np.concatenate([draw((0.3, 32000), (0.001, 16000), (0.1, 32000)), np.zeros(16000)])
    t = np.arange(96000) / 32000.0
    hum = 0.02 * np.sin(2 * np.pi * 100 * t) + draw((0.0005, 96000))
    long = draw((0.25, 40000), (0.002, 23456), (0.5, 50000), (0.05, 17777))
    return {k: v.astype(np.float32) for k, v in dict(steady=steady, speech=speech, hum=hum, long=long).items()}
