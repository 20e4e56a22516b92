"""The sentence join of include/genie_engine.h (gsv_join) stated in numpy float64: the frames' sums
of squares, the active frames, the span with its guard, the lengths at an output rate and the
pause.  Tests compare the engine against this; nothing here touches the GPU or the library."""
import math

import numpy as np

FRAME = 320     # samples of a frame: 10 ms at 32 kHz
GUARD = 640     # samples kept on either side of the active frames: 20 ms
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def threshold(trim) -> float:
    """T = 10^(trim / 10) in double, from the float32 trim widened to double."""
    return 10.0 ** (float(np.float32(trim)) / 10.0)


def frame_sums(x) -> np.ndarray:
    """Sum of the squares of every frame, in double (a float32 squared is exact there); the last
    frame may be partial."""
    x = np.asarray(x, np.float32).astype(np.float64)
    nf = (len(x) + FRAME - 1) // FRAME
    pad = np.zeros(nf * FRAME, np.float64)
    pad[:len(x)] = x
    return (pad.reshape(nf, FRAME) ** 2).sum(axis=1)


def frame_counts(n: int) -> np.ndarray:
    """Samples of every frame: 320, and what is left in the last."""
    nf = (n + FRAME - 1) // FRAME
    c = np.full(nf, FRAME, np.float64)
    if nf and n % FRAME:
        c[-1] = n % FRAME
    return c


def active(x, trim) -> np.ndarray:
    return frame_sums(x) > threshold(trim) * frame_counts(len(x))


def margin(x, trim) -> float:
    """The least relative distance of a frame's mean square from T (inf without frames): the span
    is only defined by the text where no frame lies on the threshold."""
    if len(x) == 0:
        return math.inf
    T = threshold(trim)
    return float(np.min(np.abs(frame_sums(x) / frame_counts(len(x)) - T) / T))


def span(x, trim=None):
    """(begin, end) of the speech in x; [0, n) without a trim, (0, 0) when no frame is active."""
    n = len(x)
    if trim is None:
        return 0, n
    f = np.flatnonzero(active(x, trim))
    if n == 0 or len(f) == 0:
        return 0, 0
    return max(0, FRAME * int(f[0]) - GUARD), min(n, FRAME * (int(f[-1]) + 1) + GUARD)


def audio_samples(n: int, rate: int = 32000) -> int:
    g = math.gcd(32000, rate)
    up, down = rate // g, 32000 // g
    return (n * up + down - 1) // down


def pause_samples(rate: int = 32000, pause=None) -> int:
    """(int)((double)rate * (double)pause) with the float32 pause widened to double."""
    return int(float(rate) * float(np.float32(pause or 0.0)))


def record(x, rate: int = 32000, pause=None, trim=None):
    """The span record {begin, end, n_speech, n_out} of x at `rate`."""
    b, e = span(x, trim)
    n_speech = audio_samples(e - b, rate)
    return b, e, n_speech, n_speech + pause_samples(rate, pause)


def join(x, pause=None, trim=None) -> np.ndarray:
    """The joined sentence at 32 kHz float32: the span of x, then the pause's zeros."""
    x = np.asarray(x, np.float32)
    b, e = span(x, trim)
    return np.concatenate([x[b:e], np.zeros(pause_samples(32000, pause), np.float32)])
