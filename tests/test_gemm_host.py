"""CPU: the GEMM oracle's own checks, the sharpness of its bar, and the host side of
gsv_debug_gemm / gsv_debug_rows (argument rejection and the dispatch rule, no HIP call)."""
import ctypes

import numpy as np
import pytest

from tests import gemm_oracle as O


# ------------------------------------------------------------------ the oracle itself
def test_split_is_exact_to_the_dropped_residual():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(4096) * np.exp(rng.uniform(-12, 8, 4096))).astype(np.float32)
    hi, lo = O.split_a(a)
    r = np.abs(a.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
    normal = np.abs(lo.astype(np.float64)) >= O.F16_MIN_NORMAL
    assert np.all(r[normal] <= 2.0 ** -22 * np.abs(a[normal]))      # two 11-bit roundings
    assert np.all(r[~normal] <= 2.0 ** -25)                          # half the subnormal spacing 2^-24
    # subnormal lo terms are kept, not flushed
    assert O.split_a(np.float32([2.0 ** -6 + 2.0 ** -24]))[1][0] == np.float16(2.0 ** -24)
    w = (rng.standard_normal(4096) / 16).astype(np.float32)
    wh, wl = O.split_w(w)
    rw = np.abs(w.astype(np.float64) - wh.astype(np.float64) - wl.astype(np.float64) / O.W_LO_SCALE)
    assert np.all(rw <= 2.0 ** -22 * np.abs(w) + 2.0 ** -36)


def test_rho_and_sequential_gemm():
    c = O.Case(5, 7, 64, seed=3)
    assert O.rho(c.C64, c.C64, c.S) == 0.0
    bumped = c.C64.copy()
    bumped[2, 3] += 1e-3 * c.S[2, 3]
    assert abs(O.rho(bumped, c.C64, c.S) - 1e-3) < 1e-12
    seq = O.gemm_f32_seq(c.A, c.W)
    ref = np.zeros((5, 7), np.float32)
    for i in range(5):
        for j in range(7):
            s = np.float32(0)
            for k in range(64):
                s = np.float32(s + np.float32(c.A[i, k] * c.W[j, k]))
            ref[i, j] = s
    assert np.array_equal(seq, ref)
    assert 0 < c.rho_seq < 64 * 2.0 ** -24


def test_emulated_split_is_f32_level():
    for K, kind in O.SPLIT_FAMILIES:
        c = O.Case(O.REF_M, O.REF_N, K, seed=11, kind=kind)
        assert c.rho(c.emulated()) <= c.bar / 4, (K, kind)


@pytest.mark.parametrize("K,kind", O.SPLIT_FAMILIES)
def test_bar_is_sharp(K, kind):
    """MARGIN * rho_seq is at most half the rho of each wrong GEMM, for every family of the GPU tests."""
    c = O.Case(O.REF_M, O.REF_N, K, seed=5, kind=kind)
    wrong = {"a_lo dropped": c.emulated(drop_a_lo=True),
             "a_lo flushed where subnormal": c.emulated(flush_a_lo=True),
             "k slice missing": c.emulated(skip_k=K - 16)}
    if kind == "w16":
        wrong["w_lo dropped"] = c.emulated(drop_w_lo=True)
    for name, C in wrong.items():
        r = c.rho(C)
        print(f"K={K} {kind}: bar {c.bar:.3g}, {name} {r:.3g}")
        assert c.bar <= 0.5 * r, (name, c.bar, r)


@pytest.mark.parametrize("D", [300, 512, 768, 1024])
def test_layernorm_bar_is_sharp(D):
    """The LayerNorm bar of tests/test_row_kernels_gpu.py (4 x the rho_ln of torch's fp32 layer_norm) is
    at most half the rho_ln of an fp32 LayerNorm with a one-pass variance E[x^2] - mean^2."""
    import torch
    rng = np.random.default_rng(D)
    v = O.ln_rows(3, D, rng)
    g = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    t = torch.nn.functional.layer_norm(torch.from_numpy(v), (D,), torch.from_numpy(g), torch.from_numpy(b), 1e-5)
    bar = 4.0 * O.ln_rho(t.numpy(), v, g, b, 1e-5)
    mean = v.sum(1, keepdims=True, dtype=np.float32) / np.float32(D)
    var = np.maximum((v * v).sum(1, keepdims=True, dtype=np.float32) / np.float32(D) - mean * mean, np.float32(0))
    wrong = (v - mean) / np.sqrt(var + np.float32(1e-5)) * g + b
    r = O.ln_rho(wrong, v, g, b, 1e-5)
    print(f"D={D}: bar {bar:.3g}, one-pass variance {r:.3g}")
    assert wrong.dtype == np.float32 and bar <= 0.5 * r


# ------------------------------------------------------------------ the hooks, host side
def _lib():
    from genie_tts_amd import engine
    return engine


P = 1 << 20     # an aligned stand-in pointer: the dry path and every rejection make no HIP call


def _form(M, N, K, **f):
    E = _lib()
    f = {"a": P, "w": P, "c": P, "lda": K, "ldw": K, "ldc": N, **f}
    return E.debug_gemm_form(M, N, K, **f)


def _rejected(M, N, K, dry=False, **f):
    """The hook's answer to a refused set: called with dry = 0 and a null stream, so a launch
    (on a machine without a GPU) would be an error of another kind."""
    E = _lib()
    f = {"a": P, "w": P, "c": P, "lda": K, "ldw": K, "ldc": N, **f}
    form = ctypes.c_int32(7)
    rc = E.lib().gsv_debug_gemm(ctypes.byref(E.gemm_desc(M, N, K, dry=dry, **f)), None, ctypes.byref(form))
    assert rc == -1 and form.value == -1, (rc, form.value)       # GSV_E_ARG, before any HIP call
    msg = E.lib().gsv_last_error().decode()
    assert msg.startswith("debug gemm: "), msg
    return msg


def test_debug_gemm_rejects_bad_arguments_without_touching_the_gpu():
    r = _rejected
    assert "null A" in r(64, 64, 128, a=0)
    assert "null W" in r(64, 64, 128, w=0)
    assert "null C" in r(64, 64, 128, c=0)
    assert "null C" in r(64, 64, 128, mode="relu_split", ch=P)
    assert "res" in r(64, 64, 128, mode="resid")
    assert "rowsq" in r(64, 64, 128, mode="vqdist", rowsq=P)
    assert "caches" in r(64, 1536, 128, mode="qkv", ldc=512, kv_tmax=64)
    assert "past tmax" in r(64, 1536, 128, mode="qkv", ldc=512, kv_k=P, kv_v=P, kv_tmax=64, kv_pos0=1)
    assert "a_bias" in r(64, 64, 128, a_nslab=2, a_slab_stride=8192)
    # k_gemm_nt's float4 / uint4 loads and its K-steps of 32
    assert "K % 32" in r(64, 64, 48, w_kind=0)
    assert "K % 32" in r(64, 64, 48, w_kind=1, ldw=48)
    assert "lda % 4" in r(64, 64, 64, w_kind=0, lda=66)
    assert "lda % 4" in r(64, 64, 64, w_kind=0, a=P + 4)
    assert "weight rows" in r(64, 64, 64, w_kind=0, ldw=66)
    assert "weight rows" in r(64, 64, 64, w_kind=0, w=P + 8)
    assert "weight rows" in r(64, 64, 64, w_kind=1, ldw=68)
    assert "lda % 4" in r(64, 64, 128, w_kind=1, lda=130)          # off the MFMA path, onto float4 loads
    assert "16-B aligned" in r(64, 64, 128, w_kind=1, a=P + 4)
    assert "16-B aligned" in r(64, 64, 128, w_kind=1, w=P + 2)
    assert "16-B aligned" in r(64, 64, 128, w_kind=2, wl=P + 2)
    assert "ldw at least K" in r(64, 64, 128, ldw=64)
    # split weights: shape, prologue, VQ distance
    assert "split weights" in r(64, 64, 96, w_kind=2, wl=P)
    assert "split weights" in r(64, 64, 128, w_kind=2, wl=P, lda=130)
    assert "split weights" in r(64, 64, 128, w_kind=2, wl=P, a_nslab=2, a_slab_stride=8192, a_bias=P)
    assert "split weights" in r(64, 64, 128, w_kind=2, wl=P, mode="vqdist", rowsq=P, colsq=P)
    assert "lo plane" in r(64, 64, 128, w_kind=2) and "lo plane" in r(64, 64, 128, w_kind=1, wl=P)
    # pre-split A off the large-M path
    assert "large-M" in r(64, 64, 128, ah=P, al=P)
    assert "large-M" in r(2048, 2048, 128, ah=P, al=P, lda=132)              # lda % 8
    assert "large-M" in r(2048, 2048, 128, ah=P, al=P, w_kind=2, wl=P)      # SplitW reads A
    assert "large-M" in r(2048, 2048, 128, ah=P, al=P, a_nslab=2, a_slab_stride=1 << 20, a_bias=P)
    assert "both planes" in r(2048, 2048, 128, ah=P)
    assert "16-B aligned" in r(2048, 2048, 128, ah=P + 2, al=P)
    # EPI_SLAB where gemm_slabs_supported is false, or on weights without a split-K kernel
    assert "EPI_SLAB" in r(64, 64, 96, mode="slab", ksplit=2, slab_stride=4096)
    assert "EPI_SLAB" in r(64, 64, 128, mode="slab", ksplit=2, slab_stride=4096, w_kind=0)
    assert "ksplit" in r(64, 64, 128, mode="slab", ksplit=0)
    assert "overlap" in r(64, 64, 128, mode="slab", ksplit=2, slab_stride=64)
    # an A prologue on a kernel that would ignore it
    assert "prologue" in r(64, 64, 96, a_nslab=2, a_slab_stride=8192, a_bias=P)
    assert "prologue" in r(64, 64, 128, w_kind=0, a_nslab=2, a_slab_stride=8192, a_bias=P)
    # a bad small_ns, wherever the shape would go
    for ns in (1, 5, -2):
        assert "small_ns" in r(64, 64, 128, small_ns=ns)
        assert "small_ns" in r(2048, 2048, 128, small_ns=ns)
    assert "mode" in r(64, 64, 128, mode=9)
    assert "positive" in r(0, 64, 128)
    # the dry path refuses the same sets
    assert "K % 32" in r(64, 64, 48, dry=True, w_kind=0)
    E = _lib()
    form = ctypes.c_int32(0)
    assert E.lib().gsv_debug_gemm(None, None, ctypes.byref(form)) == -1
    assert E.lib().gsv_debug_gemm(ctypes.byref(E.gemm_desc(1, 1, 32)), None, None) == -1


def test_gemm_form_boundaries():
    """gemm_form, the rule gemm_nt switches on, through the hook's dry path."""
    f = _form
    assert f(64, 64, 128, w_kind=0) == "generic_f32"
    assert f(64, 64, 96, w_kind=1, ldw=96) == "generic_f16"
    assert f(64, 64, 128, w_kind=1, mode="vqdist", rowsq=P, colsq=P) == "generic_f16"
    assert f(2048, 2048, 128, w_kind=1, mode="vqdist", rowsq=P, colsq=P) == "generic_f16"
    # M = 512 / 513 below the large-M threshold
    assert f(512, 64, 128) == "small_m4"
    assert f(513, 64, 128) == "x2"
    # 1023 / 1024 tiles of 64 x 64: 33 x 31 and 32 x 32; M <= 512 with 1024 tiles is large-M too
    assert f(33 * 64, 31 * 64, 128) == "x2"
    assert f(32 * 64, 32 * 64, 128) == "large_m"
    assert f(32 * 64 - 63, 32 * 64 - 63, 128) == "large_m"
    assert f(31 * 64, 32 * 64, 128) == "x2"
    assert f(512, 128 * 64, 128) == "large_m"
    assert f(512, 128 * 64 - 64, 128) == "small_m4"
    # cus below / at / above the grid (8 blocks; split-K counts its slices)
    assert f(128, 256, 128, cus=0) == "small_m4"
    assert f(128, 256, 128, cus=7) == "small_m2"
    assert f(128, 256, 128, cus=8) == "small_m4"
    assert f(128, 256, 256, cus=8, mode="slab", ksplit=2, slab_stride=1 << 20) == "small_m2"
    assert f(128, 256, 256, cus=16, mode="slab", ksplit=2, slab_stride=1 << 20) == "small_m4"
    for ns, name in ((2, "small_m2"), (3, "small_m3"), (4, "small_m4")):
        assert f(128, 256, 128, cus=7, small_ns=ns) == name
        assert f(2048, 2048, 128, small_ns=ns) == "large_m"
    # a_nslab keeps a launch on k_gemm_x2 at every size
    pro = dict(a_nslab=2, a_slab_stride=1 << 22, a_bias=P)
    assert f(5, 130, 256, **pro) == "x2"
    assert f(2048, 2048, 128, **pro) == "x2"
    # pre-split A: the large-M twin only
    assert f(2048, 2048, 128, ah=P, al=P) == "large_m_ps"
    assert f(2048, 2048, 128, ah=P, al=P, a=0) == "large_m_ps"
    # split weights: one form at every size
    for M, N in ((1, 64), (512, 64), (513, 64), (2048, 2048)):
        assert f(M, N, 128, w_kind=2, wl=P) == "split_w"
    assert f(70, 130, 768, w_kind=2, wl=P, mode="slab", ksplit=3, slab_stride=1 << 20) == "split_w"


def test_debug_rows_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()

    def r(op, rows, D, **f):
        d = E.RowsDesc()
        d.op, d.rows, d.D = E.ROW_OPS[op] if isinstance(op, str) else op, rows, D
        for k, v in {"in_": P, "out": P, "g": P, "b": P, "bias": P, "res": P, "nslab": 1, "ld": D, **f}.items():
            setattr(d, k, v)
        rc = E.lib().gsv_debug_rows(ctypes.byref(d), None)
        return rc, E.lib().gsv_last_error().decode()

    assert r("layernorm_rows", 1, 768)[0] == -1
    assert r("layernorm_rows_slabs", 1, 512, nslab=0)[0] == -1
    assert r("layernorm_rows_slabs", 1, 512, out_hi=P)[0] == -1
    assert r("layernorm_rows_d", 1, 1025)[0] == -1 and "1024" in r("layernorm_rows_d", 1, 1025)[1]
    assert r("layernorm_rows_d", 1, 768, out_hi=P, out_lo=P)[0] == -1
    assert r("layernorm_rows_d_slabs", 1, 768, bias=0)[0] == -1
    assert r("layernorm_rows_d_slabs", 4, 768, nslab=2, slab_stride=768)[0] == -1
    assert r("sumsq_rows", 1, 768, ld=700)[0] == -1
    assert r("argmin_dist_rows", 1, 0)[0] == -1
    assert r("sumsq_rows", -1, 8)[0] == -1
    assert r("sumsq_rows", 1, 8, in_=0)[0] == -1
    assert r(6, 1, 8)[0] == -1
    # rows == 0: success without a launch, for every kernel
    for op in E.ROW_OPS:
        assert r(op, 0, 512)[0] == 0, op
