"""fp64 reference, error measure and emulated split for the GEMM kernels of csrc/t2s.hip.

Plain numpy on the CPU; never imports the engine.  tests/NUMERICS.md states the measure, the bar
and the measured values.

For A (M,K) and W (N,K):  C64 = A64 W64^T,  S = |A64| |W64|^T,  rho(C) = max_ij |C - C64| / S.
The bar of a kernel result is MARGIN * rho_seq, rho_seq being the rho of an fp32 GEMM accumulated
sequentially over k on the CPU (gemm_f32_seq) on the operands' REF_M x REF_N block (`Case`).
"""
from __future__ import annotations

import copy

import numpy as np

MARGIN = 4.0
W_LO_SCALE = 2048.0          # W16_LO_SCALE (csrc/kernels.h)
REF_M, REF_N = 64, 256       # the block rho_seq is measured on
F16_MIN_NORMAL = 2.0 ** -14


def f16(x):
    """float32 -> fp16, round to nearest even, subnormals kept (numpy's conversion)."""
    return np.asarray(x, np.float32).astype(np.float16)


def split_a(a):
    """The kernels' activation split (split8): hi = fp16(a), lo = fp16(a - hi), the difference in f32."""
    a = np.asarray(a, np.float32)
    hi = f16(a)
    return hi, f16(a - hi.astype(np.float32))


def split_w(w):
    """W16 (csrc/kernels.h): hi = fp16(w), lo = fp16((w - hi) 2^11)."""
    w = np.asarray(w, np.float32)
    hi = f16(w)
    return hi, f16((w - hi.astype(np.float32)) * np.float32(W_LO_SCALE))


def flush_subnormal(h):
    """fp16 values with the subnormal ones replaced by zero."""
    h = np.asarray(h, np.float16).copy()
    h[np.abs(h.astype(np.float32)) < F16_MIN_NORMAL] = 0
    return h


def exact(A, W):
    """(C64, S) of the operands as given (any float type, read as fp64)."""
    A64, W64 = np.asarray(A, np.float64), np.asarray(W, np.float64)
    return A64 @ W64.T, np.abs(A64) @ np.abs(W64).T


def rho(C, C64, S):
    """max_ij |C - C64| / S (entries with S == 0 must be exact)."""
    err = np.abs(np.asarray(C, np.float64) - C64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(S > 0, err / S, np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def gemm_f32_seq(A, W):
    """fp32 GEMM, each product rounded to fp32 and added to an fp32 sum in order of k."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    C = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k in range(A.shape[1]):
        C += A[:, k:k + 1] * W[None, :, k]
    return C


def emulated_split(A, w_hi, w_lo=None, *, drop_a_lo=False, flush_a_lo=False, drop_w_lo=False, skip_k=None,
                   a_planes=None):
    """The kernels' stated arithmetic with fp64 accumulation: (a_hi + a_lo) w_hi + a_hi w_lo 2^-11
    (a_lo w_lo dropped).  w_hi / w_lo: fp16-valued planes (w_lo None: fp16-exact weights).  The
    keywords build the wrong GEMMs of the sharpness test: the A lo term dropped, flushed where it
    is an fp16 subnormal, the W lo plane dropped, the 16 k from skip_k on missing."""
    hi, lo = a_planes if a_planes is not None else split_a(A)
    if flush_a_lo:
        lo = flush_subnormal(lo)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    wh = np.asarray(w_hi).astype(np.float64)
    if drop_a_lo:
        lo = np.zeros_like(lo)
    if skip_k is not None:
        hi, lo, wh = hi.copy(), lo.copy(), wh.copy()
        hi[:, skip_k:skip_k + 16] = 0
        lo[:, skip_k:skip_k + 16] = 0
    C = (hi + lo) @ wh.T
    if w_lo is not None and not drop_w_lo:
        C = C + (hi @ np.asarray(w_lo).astype(np.float64).T) / W_LO_SCALE
    return C


class Case:
    """Operands of one GEMM case.  A is scale * N(0,1); W is N(0,1/K), fp16-valued (kind "f16"),
    fp32 (kind "f32") or fp32 split into W16 planes (kind "w16").  The arrays are generated at
    max(M, REF_M) x max(N, REF_N) and the case uses their leading M x N block, so that rho_seq is
    measured on a block of REF_M x REF_N entries of the same operands whatever M and N are (one
    entry's fp32 error can be zero by chance; a full-size sequential GEMM of the largest cases
    would take seconds).  A maximum over fewer entries than the case has only lowers the bar."""

    def __init__(self, M, N, K, seed=0, kind="f16", scale=1.0):
        rng = np.random.default_rng([seed, M, N, K])
        self.M, self.N, self.K, self.kind = M, N, K, kind
        self.A_all = (rng.standard_normal((max(M, REF_M), K)) * scale).astype(np.float32)
        w = (rng.standard_normal((max(N, REF_N), K)) / np.sqrt(K)).astype(np.float32)
        if kind == "f16":
            w = f16(w).astype(np.float32)
        self.W_all = w
        self.A, self.W = self.A_all[:M], self.W_all[:N]
        self.w_hi, self.w_lo = (None, None)
        if kind == "w16":
            self.w_hi, self.w_lo = (p[:N] for p in split_w(w))
        elif kind == "f16":
            self.w_hi = f16(w)[:N]
        self.C64, self.S = exact(self.A, self.W)
        self._rho_seq = None

    def with_A(self, A_all, M=None):
        """This case with other activations (at least REF_M rows; the first M are used)."""
        c = copy.copy(self)
        c.M = self.M if M is None else M
        c.A_all = np.asarray(A_all, np.float32)
        assert c.A_all.shape[0] >= max(c.M, 1) and c.A_all.shape[1] == self.K
        c.A = c.A_all[:c.M]
        c.C64, c.S = exact(c.A, c.W)
        c._rho_seq = None
        return c

    @property
    def rho_seq(self):
        if self._rho_seq is None:
            a, w = self.A_all[:REF_M], self.W_all[:REF_N]
            self._rho_seq = rho(gemm_f32_seq(a, w), *exact(a, w))
        return self._rho_seq

    @property
    def bar(self):
        return MARGIN * self.rho_seq

    def rho(self, C):
        return rho(C, self.C64, self.S)

    def emulated(self, **kw):
        """The emulated split of this case (kinds "f16" and "w16")."""
        return emulated_split(self.A, self.w_hi, self.w_lo, **kw)


# ------------------------------------------------------------------ LayerNorm (tests/test_row_kernels_gpu.py)
def ln64(v, g, b, eps):
    """(LayerNorm over the last axis in fp64, the rows' fp64 variance)."""
    v = np.asarray(v).astype(np.float64)
    mean = v.mean(1, keepdims=True)
    var = ((v - mean) ** 2).mean(1, keepdims=True)
    return (v - mean) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64), var


def ln_rho(out, v, g, b, eps):
    """max |out - ref| / (|g| mean|v| / sqrt(var + eps) + |ref|): the error of a LayerNorm output in
    units of what one rounding of the row's mean does to it, plus the output itself (the analogue
    of the GEMM's rho: a maximum over rows of different conditioning means something)."""
    ref, var = ln64(v, g, b, eps)
    scale = np.abs(np.asarray(g, np.float64)) * np.abs(np.asarray(v).astype(np.float64)).mean(1, keepdims=True) \
        / np.sqrt(var + eps)
    return float(np.max(np.abs(np.asarray(out).astype(np.float64) - ref) / (scale + np.abs(ref))))


def ln_rows(rows, D, rng, const=0.75):
    """rows == 3: N(0,1), a constant (sums of up to 1024 copies of 0.75 are exact in fp32, so its
    output is b exactly), and 1e3 + N(0,1) (where a one-pass variance fails); fewer: N(0,1)."""
    x = rng.standard_normal((rows, D)).astype(np.float32)
    if rows == 3:
        x[1] = const
        x[2] += np.float32(1e3)
    return x


# (K, weight kind) of every shape family the GPU tests use on the split-activation kernels
SPLIT_FAMILIES = [(128, "f16"), (256, "f16"), (384, "f16"), (640, "f16"), (768, "f16"),
                  (128, "w16"), (768, "w16")]
