"""fp64 references, error bars and wrong convs for the vocoder kernels of csrc/vits*.hip.

Plain numpy / torch on the CPU; never imports the engine.  A conv is turned into the GEMM
A (n_t x Cin K) W^T (Cout x Cin K) by im2col, so `exact`, `rho`, `gemm_f32_seq`, `split_a` and
`emulated_split` of tests/gemm_oracle.py apply unchanged, and the bar is NUMERICS.md's
4 * rho_seq on a 64 x 256 block of the case's own im2col operands.
"""
from __future__ import annotations

import numpy as np

from tests import gemm_oracle as G

EPS = 2.0 ** -24          # one fp32 rounding, relative
MODES = ("store", "relu", "resid", "vec", "sub", "tanh", "acc_first", "acc_add", "acc_mean", "resid_vec",
         "split_resid")


def lrelu32(x, slope):
    """The kernels' input activation in fp32: x < 0 ? x * slope : x."""
    x = np.asarray(x, np.float32)
    return np.where(x < 0, x * np.float32(slope), x).astype(np.float32)


def im2col64(x, K, dil, pad, n_t):
    """im2col of fp64 values as they are (an intermediate of a reference, or a tolerance)."""
    x = np.asarray(x, np.float64)
    Cin, Tin = x.shape
    A = np.zeros((n_t, Cin, K))
    t = np.arange(n_t)
    for j in range(K):
        src = t + j * dil - pad
        ok = (src >= 0) & (src < Tin)
        A[ok, :, j] = x[:, src[ok]].T
    return A.reshape(n_t, Cin * K)


def im2col(x, K, dil, pad, n_t, in_act=False, slope=0.1, in_scale=None):
    """x (Cin, Tin) -> A (n_t, Cin K), A[t, ci K + j] = s[ci] act(x)[ci, t + j dil - pad], zero outside
    [0, Tin): the conv of ConvArgs (csrc/vits.h) as the left operand of a GEMM with w.reshape(Cout, Cin K).
    The activation and the input scale are applied in fp32, as the kernels apply them."""
    x = np.asarray(x, np.float32)
    if in_act:
        x = lrelu32(x, slope)
    if in_scale is not None:
        x = (x * np.asarray(in_scale, np.float32)[:, None]).astype(np.float32)
    Cin, Tin = x.shape
    A = np.zeros((n_t, Cin, K), np.float32)
    t = np.arange(n_t)
    for j in range(K):
        src = t + j * dil - pad
        ok = (src >= 0) & (src < Tin)
        A[ok, :, j] = x[:, src[ok]].T
    return A.reshape(n_t, Cin * K)


def polyphase(w, u):
    """ConvTranspose1d weight w (Cin, Cout, k), stride u -> W_r (u, Cout, Cin, M), M = ceil(k / u):
    W_r[co][ci][j] = w[ci][co][r + (M - 1 - j) u] (0 past k); phase r of the output, column t u + r of
    the unpadded transpose, is the M-tap conv of x with W_r at pad M - 1."""
    w = np.asarray(w)
    Cin, Cout, k = w.shape
    M = (k + u - 1) // u
    W = np.zeros((u, Cout, Cin, M), w.dtype)
    for r in range(u):
        for j in range(M):
            kk = r + (M - 1 - j) * u
            if kk < k:
                W[r, :, :, j] = w[:, :, kk].T
    return W


def conv_transpose64(x, w, u, pad):
    """torch's fp64 conv_transpose1d of x (Cin, Tin) with w (Cin, Cout, k): the polyphase reference."""
    import torch
    import torch.nn.functional as F
    y = F.conv_transpose1d(torch.from_numpy(np.asarray(x, np.float64))[None], torch.from_numpy(np.asarray(w, np.float64)),
                           stride=u, padding=pad)
    return y[0].numpy()


class ConvCase:
    """Operands of one conv.  x ~ x_scale N(0,1) (Cin, Tin); w ~ N(0, 1/(Cin K)) (Cout, Cin, K), fp16-valued
    with a per-channel scale in 0.5 .. 1.5 for kind "f16"; bias ~ 0.1 N(0,1).  v64 (Cout, n_t) is the fp64
    conv with bias, tol its tolerance: bar S (times |scale|), one fp32 rounding of the scale multiply and
    one of the bias add.  The operand arrays are generated long and tall enough that a 64 x 256 block of
    im2col rows and weight rows exists; the case uses their leading part."""

    def __init__(self, Cin, Cout, K, Tin, dil=1, pad=None, n_t=None, seed=0, kind="f32", in_act=False,
                 slope=0.1, x_scale=1.0, bias=True, x=None):
        rng = np.random.default_rng([seed, Cin, Cout, K, Tin, dil])
        self.Cin, self.Cout, self.K, self.Tin, self.dil, self.kind = Cin, Cout, K, Tin, dil, kind
        self.pad = dil * (K - 1) // 2 if pad is None else pad
        self.n_t = Tin + 2 * self.pad - dil * (K - 1) if n_t is None else n_t
        self.in_act, self.slope = in_act, slope
        t_all = max(Tin, G.REF_M + dil * (K - 1))
        self.x_all = (rng.standard_normal((Cin, t_all)) * x_scale).astype(np.float32)
        if x is not None:
            self.x_all[:, :Tin] = x
        w = (rng.standard_normal((max(Cout, G.REF_N), Cin, K)) / np.sqrt(Cin * K)).astype(np.float32)
        if kind == "f16":
            w = G.f16(w).astype(np.float32)
        self.w_all = w
        self.x, self.w = np.ascontiguousarray(self.x_all[:, :Tin]), np.ascontiguousarray(w[:Cout])
        self.scale = (rng.random(Cout) + 0.5).astype(np.float32) if kind == "f16" else np.ones(Cout, np.float32)
        self.bias = (0.1 * rng.standard_normal(Cout)).astype(np.float32) if bias else None
        self.A = im2col(self.x, K, dil, self.pad, self.n_t, in_act, slope)
        self.Wm = self.w.reshape(Cout, Cin * K)
        a_ref = im2col(self.x_all, K, dil, self.pad, G.REF_M, in_act, slope)
        w_ref = w[:G.REF_N].reshape(-1, Cin * K)
        self.rho_seq = G.rho(G.gemm_f32_seq(a_ref, w_ref), *G.exact(a_ref, w_ref))
        self.bar = G.MARGIN * self.rho_seq
        C64, S = G.exact(self.A, self.Wm)
        self.C64, self.S = C64.T, S.T                                   # (Cout, n_t)
        self.v64, self.tol = self.finish(self.C64, self.S)

    def finish(self, C64, S):
        """(sum, S) (Cout, n) -> (v64, tol): the scale, the bias, and their roundings."""
        sc = self.scale.astype(np.float64)[:, None]
        v = C64 * sc
        tol = self.bar * S * np.abs(sc)
        if self.kind == "f16":
            tol = tol + EPS * np.abs(v)
        if self.bias is not None:
            v = v + self.bias.astype(np.float64)[:, None]
            tol = tol + EPS * np.abs(v)
        return v, tol

    def wh(self):
        """The f16 path's weights [Cout][K][Cin] as fp16."""
        return np.ascontiguousarray(G.f16(self.w).transpose(0, 2, 1))

    def emulated(self, **kw):
        """The kernels' stated split arithmetic (gemm_oracle.emulated_split) with scale and bias, (Cout, n_t)."""
        C = G.emulated_split(self.A, G.f16(self.Wm), **kw).T * self.scale.astype(np.float64)[:, None]
        return C + (self.bias.astype(np.float64)[:, None] if self.bias is not None else 0.0)

    def rho(self, out):
        """rho of a kernel's pre-epilogue values (bias and scale taken back out)."""
        o = np.asarray(out, np.float64)
        if self.bias is not None:
            o = o - self.bias.astype(np.float64)[:, None]
        return G.rho(o / self.scale.astype(np.float64)[:, None], self.C64, self.S)


def tanh_err(v64):
    """The worst error of torch's CPU fp32 tanh against fp64 on the fp32 pre-activations."""
    import torch
    v = np.asarray(v64, np.float64).astype(np.float32)
    return float(np.max(np.abs(torch.tanh(torch.from_numpy(v)).numpy().astype(np.float64) - np.tanh(v.astype(np.float64)))))


def epilogue(mode, v, tol, *, res=None, vec=None, acc=None, div=1.0, split=0, res2=None):
    """The ConvMode epilogue in fp64 on v (Cout, n) with its tolerance carried through: every stated add
    (and the divide) contributes one fp32 rounding of its result; relu and tanh are 1-Lipschitz; tanh adds
    4 x torch's fp32 tanh error.  Returns {buffer name: (ref, tol)} for the buffers the mode writes
    ("out", "acc", "out2")."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    res, acc, res2 = f(res), f(acc), f(res2)
    vec = None if vec is None else np.asarray(vec, np.float64).reshape(-1, 1) if np.ndim(vec) == 1 else f(vec)

    def add(a, b, t):
        s = a + b
        return s, t + EPS * np.abs(s)

    if mode == "store":
        return {"out": (v, tol)}
    if mode == "relu":
        return {"out": (np.maximum(v, 0), tol)}
    if mode == "resid":
        return {"out": add(res, v, tol)}
    if mode == "vec":
        return {"out": add(v, vec, tol)}
    if mode == "sub":
        return {"out": add(res, -v, tol)}
    if mode == "tanh":
        return {"out": (np.tanh(v), tol + 4.0 * tanh_err(v))}
    if mode == "acc_first":
        return {"acc": add(res, v, tol)}
    if mode == "acc_add":
        return {"acc": add(acc, *add(res, v, tol))}
    if mode == "acc_mean":
        s, t = add(acc, *add(res, v, tol))
        o = s / div
        return {"out": (o, t / abs(div) + EPS * np.abs(o))}
    if mode == "resid_vec":
        s, t = add(res, v, tol)
        return {"out": add(s, vec, t)}
    if mode == "split_resid":
        return {"out": add(res[:split], v[:split], tol[:split]), "out2": add(res2, v[split:], tol[split:])}
    raise ValueError(mode)


# ------------------------------------------------------------------ wrong convs (the sharpness test)
def wrong_convs(c: ConvCase, tile=64):
    """rho-ready pre-epilogue sums (Cout, n_t) of convs that are wrong the way a kernel could be: the lo term
    dropped, flushed where subnormal, the last tap missing, one 8-channel group of one tap missing, the
    first halo column of every `tile`-column tile read as zero."""
    wh = G.f16(c.Wm)
    out = {"lo dropped": G.emulated_split(c.A, wh, drop_a_lo=True).T,
           "lo flushed where subnormal": G.emulated_split(c.A, wh, flush_a_lo=True).T}
    A3 = c.A.reshape(c.n_t, c.Cin, c.K).copy()
    A3[:, :, c.K - 1] = 0
    out["one tap missing"] = G.emulated_split(A3.reshape(c.n_t, -1), wh).T
    A3 = c.A.reshape(c.n_t, c.Cin, c.K).copy()
    A3[:, c.Cin - 8:, 0] = 0
    out["one 8-channel group missing"] = G.emulated_split(A3.reshape(c.n_t, -1), wh).T
    if c.K > 1:
        # tile t0's first staged column is input time t0 - pad: tap 0 of output t0
        A3 = c.A.reshape(c.n_t, c.Cin, c.K).copy()
        A3[::tile, :, 0] = 0
        out["first halo column read as zero"] = G.emulated_split(A3.reshape(c.n_t, -1), wh).T
    return out


# ------------------------------------------------------------------ attention
def _mha_dense(tq, tk, tv, heads, dk, sc, postdiv, tek, tev, window, ir0):
    """Attention of the query rows tq over the keys tk (torch, one dtype); row m sits at index ir0 + m of the
    keys' sequence for the rel-pos terms."""
    import torch
    nq, nk = tq.shape[0], tk.shape[0]
    out = torch.zeros((nq, heads * dk), dtype=tq.dtype)
    rows = torch.arange(nq)
    for h in range(heads):
        c = slice(h * dk, (h + 1) * dk)
        qh = tq[:, c] if postdiv else tq[:, c] / sc
        s = qh @ tk[:, c].T
        if postdiv:
            s = s / sc
        band = []
        if tek is not None or tev is not None:
            for r in range(2 * window + 1):
                j = rows + ir0 + r - window
                ok = (j >= 0) & (j < nk)
                band.append((r, rows[ok], j[ok]))
        if tek is not None:
            qe = qh @ tek.T
            for r, i, j in band:
                s[i, j] = s[i, j] + qe[i, r]
        p = torch.softmax(s, 1)
        o = p @ tv[:, c]
        if tev is not None:
            for r, i, j in band:
                o[i] = o[i] + p[i, j][:, None] * tev[r][None, :]
        out[:, c] = o
    return out


def mha_ref(q, k, v, heads, dk, scale, postdiv=False, ek=None, ev=None, window=0, ranges=None, dtype=np.float64):
    """Softmax attention with the rel-pos key and value terms (MhaArgs, csrc/vits.h) on q (nq, heads dk),
    k, v (nk, heads dk) in `dtype` (fp64: the reference; torch fp32 on the CPU: what the bar is measured
    on).  ranges[i] = (first key, key count) of row i (packed sequences; with rel-pos terms row i is
    key i), else every key."""
    import torch
    td = torch.float64 if dtype == np.float64 else torch.float32
    tq, tk, tv = (torch.from_numpy(np.asarray(a, np.float32)).to(td) for a in (q, k, v))
    tek = None if ek is None else torch.from_numpy(np.asarray(ek, np.float32)).to(td)
    tev = None if ev is None else torch.from_numpy(np.asarray(ev, np.float32)).to(td)
    sc = torch.tensor(scale, dtype=td)
    if ranges is None:
        return _mha_dense(tq, tk, tv, heads, dk, sc, postdiv, tek, tev, window, 0).numpy()
    out = torch.zeros((tq.shape[0], heads * dk), dtype=td)
    i = 0
    while i < tq.shape[0]:                       # runs of rows with one key range
        s0, cnt = int(ranges[i][0]), int(ranges[i][1])
        e = i
        while e < tq.shape[0] and (int(ranges[e][0]), int(ranges[e][1])) == (s0, cnt):
            e += 1
        out[i:e] = _mha_dense(tq[i:e], tk[s0:s0 + cnt], tv[s0:s0 + cnt], heads, dk, sc, postdiv, tek, tev, window, i - s0)
        i = e
    return out.numpy()


# ------------------------------------------------------------------ LayerNorm over channels
def ln_channels_rho(out, v, g, b):
    """rho_ln (gemm_oracle.ln_rho) of a [C][T] LayerNorm over C: the columns are the rows."""
    return G.ln_rho(np.asarray(out).T, np.asarray(v).T, g, b, 1e-5)


def seg_fill_ref(n, off, ln, f):
    """seg[t] = i with off[i] f <= t < (off[i] + len[i]) f, else -1."""
    seg = np.full(n, -1, np.int32)
    for i, (o, l) in enumerate(zip(off, ln)):
        seg[o * f:min(n, (o + l) * f)] = i
    return seg
