"""fp64 / fp32 references and bars for the T2S decoder's own kernels (csrc/t2s.hip attention and
GEMV, csrc/t2s_decode.hip).  Plain numpy / torch on the CPU; never imports the engine.
tests/NUMERICS.md states the measures, the bars and the measured values.

Attention of one query row over keys [0, len) of its sequence, per head of 32 dims, as the graph
states it: scores (q s)(k s), softmax, P V.  The caches are [16][tmax][32].
"""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import gemm_oracle as G

MARGIN = G.MARGIN
HEADS, DK = 16, 32
SCALE = math.sqrt(1.0 / math.sqrt(32.0))      # applied to q and to k separately (stage #91-94)
BAR_ROWS, BAR_MIN_KEYS = 8, 64                # the rows an attention bar is measured on
FX = 4294967296.0                             # the fixed-point hand-off's 2^32 (csrc/common.h)
LN_EPS = 1e-5
LOG2E = np.float32(1.4426950408889634)        # __expf(x) = exp2(x * log2(e)) with the product in fp32

WRONG = ("drop_last", "one_more", "drop_64", "no_new_row", "skip_rescale", "q_scale_only")


def _exp(x, mode):
    if mode == "fast_exp":
        return np.exp2((x * LOG2E).astype(np.float32)).astype(np.float32)
    return np.exp(x)


def attn_row(q, K, V, length, scale=SCALE, mode="f64", wrong=None):
    """softmax((q s)(K s)^T) V of one row: q [16][32], K / V [16][T][32], keys [0, length) -> [16][32].
    mode "f64", "f32" (every operation in fp32) or "fast_exp" (fp32 with exp(x) = exp2 of the fp32
    product x log2(e), the device's __expf).  wrong: one of WRONG, the defects of the sharpness test."""
    dt = np.float64 if mode == "f64" else np.float32
    s = dt(scale)
    if wrong == "drop_last":
        length -= 1
    elif wrong == "one_more":
        length += 1
    assert 1 <= length <= K.shape[1]
    q, K, V = np.asarray(q).astype(dt), np.asarray(K)[:, :length].astype(dt), np.asarray(V)[:, :length].astype(dt)
    if wrong == "drop_64":
        assert length > 64
        K, V = np.delete(K, 64, axis=1), np.delete(V, 64, axis=1)
    if wrong == "no_new_row":          # a zeroed cache row read in place of the appended one
        K, V = K.copy(), V.copy()
        K[:, -1], V[:, -1] = 0, 0
    ks = K if wrong == "q_scale_only" else K * s
    sc = np.einsum("hd,htd->ht", q * s, ks).astype(dt)
    if wrong == "skip_rescale":
        # online softmax over 64-key chunks whose rescale of the running sum and output by
        # exp(m_old - m_new) is left out at the second chunk
        assert length > 64
        m = sc[:, :64].max(1)
        p = np.exp(sc[:, :64] - m[:, None])
        l, o = p.sum(1), np.einsum("ht,htd->hd", p, V[:, :64])
        for k0 in range(64, sc.shape[1], 64):
            c = sc[:, k0:k0 + 64]
            mn = np.maximum(m, c.max(1))
            corr = np.ones_like(m) if k0 == 64 else np.exp(m - mn)
            p = np.exp(c - mn[:, None])
            l, o, m = l * corr + p.sum(1), o * corr[:, None] + np.einsum("ht,htd->hd", p, V[:, k0:k0 + 64]), mn
        return o / l[:, None]
    p = _exp((sc - sc.max(1, keepdims=True)).astype(dt), mode)
    p = (p / p.sum(1, keepdims=True, dtype=dt)).astype(dt)
    return np.einsum("ht,htd->hd", p, V).astype(dt)


def attn_rows(q, K, V, lens, scale=SCALE, mode="f64", wrong=None):
    """attn_row of every row r of q [R][512] over keys [0, lens[r]) -> [R][512]."""
    q = np.asarray(q).reshape(len(lens), HEADS, DK)
    return np.stack([attn_row(q[r], K, V, int(lens[r]), scale, mode, wrong).reshape(HEADS * DK)
                     for r in range(len(lens))])


class Family:
    """The inputs of the attention cases: q, k, v ~ qk * N(0,1) (v always N(0,1)); qk = 1 is the
    unit-scale family, qk = 4 the peaked one (scores reach tens).  A family is one generator: the
    cases draw their rows and caches from it and its bar is measured on it."""

    def __init__(self, qk=1.0, seed=0):
        self.qk, self.seed = float(qk), seed

    @functools.lru_cache(maxsize=None)
    def data(self, rows, nseq, tmax):
        """(q [rows][512], K, V [nseq][16][tmax][32]) in fp32."""
        rng = np.random.default_rng([self.seed, int(self.qk * 16), rows, nseq, tmax])
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        q, K, V = f(rows, 512) * np.float32(self.qk), f(nseq, HEADS, tmax, DK) * np.float32(self.qk), f(nseq, HEADS, tmax, DK)
        for a in (q, K, V):
            a.setflags(write=False)
        return q, K, V

    @functools.lru_cache(maxsize=None)
    def err(self, T, mode, wrong=None):
        """Per row, the worst |result - fp64| of BAR_ROWS rows of lengths T .. T - 7 (T raised so that
        every row has at least BAR_MIN_KEYS keys); result = the fp32 computation `mode`, or with
        `wrong` the fp64 computation with that defect."""
        T = max(T, BAR_MIN_KEYS + BAR_ROWS)      # the shortest row has 65 keys: a second chunk exists
        q, K, V = self.data(BAR_ROWS, 1, T + 1)
        lens = [T - i for i in range(BAR_ROWS)]
        ref = attn_rows(q, K[0], V[0], lens)
        got = attn_rows(q, K[0], V[0], lens, mode="f64" if wrong else mode, wrong=wrong)
        return np.abs(got.astype(np.float64) - ref).max(1)

    def bar(self, T, mode, margin=MARGIN):
        """margin x the worst absolute error of the CPU fp32 computation `mode` against fp64: a case
        whose own length has one key (where fp32 is exact) still gets the bar of 64 keys or more."""
        return margin * float(self.err(T, mode).max())


UNIT, PEAKED = Family(1.0), Family(4.0)
# bar mode of each kernel: the three online-softmax prefill kernels use __expf
BAR_MODE = {"rows": "f32", "dec_slabs": "f32", "attn_out": "f32", "flash": "fast_exp", "rowlane": "fast_exp",
            "mf32": "fast_exp"}
# kernel-specific margins (tests/NUMERICS.md says why where one is not MARGIN; at most 16)
KERNEL_MARGIN = {k: MARGIN for k in BAR_MODE}


# ------------------------------------------------------------------ fused decode-step kernels
def f16w(rng, n, k, scale=None):
    """fp16-valued N(0, 1/k) weights [n][k] as float32."""
    return G.f16(rng.standard_normal((n, k)) * (scale if scale is not None else 1.0 / np.sqrt(k))).astype(np.float32)


def outproj_part64(o, WoT):
    """part[h][n] = sum_d WoT[32 h + d][n] o[h][d]: o [16][32] -> [16][512] (fp64), and S = |o| |WoT|."""
    o64, W = np.asarray(o, np.float64), np.asarray(WoT, np.float64).reshape(HEADS, DK, 512)
    return np.einsum("hd,hdn->hn", o64, W), np.einsum("hd,hdn->hn", np.abs(o64), np.abs(W))


def group_rho_seq(a, w):
    """rho_seq (gemm_oracle) of a stack of short GEMVs on their own operands: a [G][M][K] activations
    and w [G][K][N] weights, each product rounded to fp32 and added to an fp32 sum in order of k,
    against fp64 with S = |a| |w|; the worst entry of all groups.  The bar's unit for the 32- / 64-term
    stages (one head of the out-projection, one slice of FFN2)."""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    C = np.zeros((a.shape[0], a.shape[1], w.shape[2]), np.float32)
    for k in range(a.shape[2]):
        C += a[:, :, k, None] * w[:, k, None, :]
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    return G.rho(C, np.einsum("gmk,gkn->gmn", a64, w64), np.einsum("gmk,gkn->gmn", np.abs(a64), np.abs(w64)))


def fx(v):
    """to_fx (csrc/common.h): rint(double(v) 2^32) as int64."""
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * FX).astype(np.int64)


def from_fx(a):
    """from_fx: float(double(a) 2^-32)."""
    return (np.asarray(a, np.int64).astype(np.float64) / FX).astype(np.float32)


def ln_bar(v, g, b):
    """MARGIN x rho_ln of torch's fp32 layer_norm on the CPU on the same rows (NUMERICS.md, row kernels)."""
    import torch
    v = np.ascontiguousarray(v, np.float32)
    t = torch.nn.functional.layer_norm(torch.from_numpy(v), (v.shape[1],), torch.from_numpy(np.asarray(g, np.float32)),
                                       torch.from_numpy(np.asarray(b, np.float32)), LN_EPS).numpy()
    return MARGIN * G.ln_rho(t, v, g, b, LN_EPS)


def ffn_ref(x, W1, b1, W2T, nslices):
    """From LN1's output x [B][512] (the values given, read as fp64): f = relu(W1 x + b1) [B][2048] with
    S1 = |x| |W1|^T, and per slice j the partial part[j][b][n] = sum_{r in slice} W2T[r][n] f[b][r]
    with S2[j] = |f| |W2T| over the slice."""
    x64, W1, W2T = np.asarray(x, np.float64), np.asarray(W1, np.float64), np.asarray(W2T, np.float64)
    pre = x64 @ W1.T + np.asarray(b1, np.float64)
    S1 = np.abs(x64) @ np.abs(W1).T + np.abs(np.asarray(b1, np.float64))
    f = np.maximum(pre, 0.0)
    rpb = 2048 // nslices
    fs, Ws = f.reshape(-1, nslices, rpb), W2T.reshape(nslices, rpb, 512)
    part = np.einsum("bjr,jrn->jbn", fs, Ws)
    S2 = np.einsum("bjr,jrn->jbn", np.abs(fs), np.abs(Ws))
    return f, S1, part, S2, np.abs(Ws)
