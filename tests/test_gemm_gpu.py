"""GPU: every kernel behind gemm_nt (csrc/t2s.hip), one launch at a time through gsv_debug_gemm,
against the fp64 reference of tests/gemm_oracle.py.  The bar is MARGIN * rho_seq (tests/NUMERICS.md);
every case asserts the form the hook reports, and every launch runs with NaN in the padding of A and
W and a sentinel around C (`launch`)."""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_oracle as O

pytestmark = pytest.mark.gpu

SENT = 12344.0      # exact in fp16 too (the RELU_SPLIT planes)
ULP = 2.0 ** -23


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _padded(x, rows_extra, ld, fill=float("nan")):
    """x (R, C) in an allocation of (R + rows_extra, ld) whose other cells hold `fill`."""
    out = np.full((x.shape[0] + rows_extra, ld), fill, x.dtype)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def launch(c, expect, mode="store", *, k0=0, k1=None, rows=None, ldc=None, a_planes=None, **f):
    """One gemm_nt launch of case `c` (its K slice [k0, k1) and first `rows` rows, if given).
    A and W sit in allocations with 8 NaN padding columns and 3 NaN rows past M / N; C has 5 pad
    columns and 2 rows past M holding SENT, which must survive.  Returns C[:M, :N] (numpy), or for
    mode "slab" the [ksplit, M, N] slabs, or for "relu_split" the (hi, lo) planes."""
    from genie_tts_amd.engine import debug_gemm
    M, N, K = rows or c.M, c.N, c.K
    k1 = K if k1 is None else k1
    ld = K + 8
    A = _dev(_padded(c.A[:M], 3, ld))
    f = dict(f)
    keep = [A]
    if c.kind == "f32":
        W = _dev(_padded(c.W, 3, ld))
        f.update(w=W[:, k0:], w_kind=0)
    elif c.kind == "f16":
        W = _dev(_padded(c.w_hi, 3, ld))
        f.update(w=W[:, k0:], w_kind=1)
    else:
        W, Wl = _dev(_padded(c.w_hi, 3, ld)), _dev(_padded(c.w_lo, 3, ld))
        keep.append(Wl)
        f.update(w=W[:, k0:], wl=Wl[:, k0:], w_kind=2)
    if a_planes is not None:
        ah, al = (_dev(_padded(p[:M], 3, ld)) for p in a_planes)
        keep += [ah, al]
        f.update(ah=ah[:, k0:], al=al[:, k0:])
    ldc = N + 5 if ldc is None else ldc
    nz = f.get("ksplit", 1) if mode == "slab" else 1
    half = mode == "relu_split"
    C = torch.full((nz, M + 2, ldc), SENT, dtype=torch.float32, device="cuda")
    if half:
        Ch, Cl = (torch.full((M + 2, ldc), SENT, dtype=torch.float16, device="cuda") for _ in range(2))
        f.update(ch=Ch, cl=Cl)
    if mode == "slab":
        f.update(slab_stride=(M + 2) * ldc)
    for k, v in list(f.items()):
        if isinstance(v, np.ndarray):
            f[k] = _dev(v)
            keep.append(f[k])
    form = debug_gemm(M, N, k1 - k0, a=A[:, k0:], lda=ld, ldw=ld, c=None if half else C, ldc=ldc, mode=mode, **f)
    torch.cuda.synchronize()
    assert form == expect, (form, expect)
    outs = [t.float().cpu().numpy() for t in ((Ch, Cl) if half else (C,))]
    for o in outs:
        o = o.reshape(-1, M + 2, ldc)
        assert np.all(o[:, M:, :] == SENT) and np.all(o[:, :M, N:] == SENT), "wrote outside C[:M, :N]"
        if mode != "qkv":
            assert np.all(np.isfinite(o[:, :M, :N])), "padding leaked into the result"
    if half:
        return tuple(o[:M, :N] for o in outs)
    out = outs[0].reshape(nz, M + 2, ldc)[:, :M, :N]
    return out if mode == "slab" else out[0]


def check_rho(c, C, what):
    r = c.rho(C)
    print(f"RHO {what} M={c.M} N={c.N} K={c.K}: rho {r:.3g} bar {c.bar:.3g}")
    assert r <= c.bar, (what, r, c.bar)


@functools.lru_cache(maxsize=None)
def case(M, N, K, kind="f16", seed=0, scale=1.0):
    return O.Case(M, N, K, seed=seed, kind=kind, scale=scale)


# ------------------------------------------------------------------ generic kernels
@pytest.mark.parametrize("kind,form", [("f32", "generic_f32"), ("f16", "generic_f16")])
@pytest.mark.parametrize("M,N,K", [(1, 1, 32), (37, 70, 96), (65, 129, 160)])
def test_generic(M, N, K, kind, form):
    c = case(M, N, K, kind)
    check_rho(c, launch(c, form), form)


# ------------------------------------------------------------------ small-M ring
SMALL = [(1, 1, 128, 2), (65, 63, 256, 2), (31, 65, 640, 2),
         (64, 1025, 128, 3), (1, 65, 256, 3), (65, 63, 640, 3),
         (512, 63, 128, 4), (31, 1, 256, 4), (65, 65, 640, 4)]


@pytest.mark.parametrize("M,N,K,ns", SMALL)
def test_small_m_forced_depth(M, N, K, ns):
    c = case(M, N, K)
    check_rho(c, launch(c, f"small_m{ns}", small_ns=ns), f"small_m{ns}")


def test_small_m_depth_by_rule():
    c = case(65, 65, 256)
    check_rho(c, launch(c, "small_m2", cus=1), "small_m2 (cus=1)")
    c = case(65, 1025, 640)
    check_rho(c, launch(c, "small_m4", cus=0), "small_m4 (cus=0)")


# ------------------------------------------------------------------ k_gemm_x2
def test_x2_odd_tail():
    c = case(513, 64, 384)
    check_rho(c, launch(c, "x2"), "x2")


def test_x2_slab_prologue():
    """A = relu(a_bias + the sum of 3 slabs in slab order, in fp32)."""
    M, N, K, nz = 5, 130, 256, 3
    rng = np.random.default_rng(7)
    slabs = rng.standard_normal((nz, O.REF_M, K)).astype(np.float32)
    a_bias = rng.standard_normal(K).astype(np.float32)
    acc = slabs[0].copy()
    for z in range(1, nz):
        acc = acc + slabs[z]
    A = np.maximum(a_bias[None, :] + acc, np.float32(0))
    assert A.dtype == np.float32
    c = case(M, N, K)
    c2 = c.with_A(A)
    ld = K + 8
    buf = np.full((nz, M + 3, ld), np.nan, np.float32)
    buf[:, :M, :K] = slabs[:, :M]
    from genie_tts_amd.engine import debug_gemm
    Ad, Wd, bd = _dev(buf), _dev(_padded(c.w_hi, 3, ld)), _dev(a_bias)
    C = torch.full((M + 2, N + 5), SENT, device="cuda")
    form = debug_gemm(M, N, K, a=Ad, lda=ld, w=Wd, ldw=ld, c=C, ldc=N + 5, a_nslab=nz, a_slab_stride=(M + 3) * ld,
                      a_bias=bd, a_relu=1)
    torch.cuda.synchronize()
    assert form == "x2"
    out = C.cpu().numpy()
    assert np.all(out[M:] == SENT) and np.all(out[:, N:] == SENT) and np.all(np.isfinite(out[:M, :N]))
    check_rho(c2, out[:M, :N], "x2 (slab prologue)")


# ------------------------------------------------------------------ large-M
LARGE = [(1000, 4090, 128), (1030, 3900, 384)]     # 16 x 64 = 1024 tiles; 17 x 61 = 1037, nwg % 8 == 5


@functools.lru_cache(maxsize=None)
def large_result(i, presplit):
    c = case(*LARGE[i])
    if presplit:
        return launch(c, "large_m_ps", a_planes=O.split_a(c.A))
    return launch(c, "large_m")


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("presplit", [False, True])
def test_large_m(i, presplit):
    c = case(*LARGE[i])
    check_rho(c, large_result(i, presplit), "large_m_ps" if presplit else "large_m")


# ------------------------------------------------------------------ split weights
@pytest.mark.parametrize("K", [128, 768])
@pytest.mark.parametrize("M,N", [(1, 130), (70, 130), (1, 192), (70, 192)])
def test_split_w(M, N, K):
    c = case(M, N, K, "w16")
    check_rho(c, launch(c, "split_w"), "split_w")


# ------------------------------------------------------------------ bit-identity claims
def test_x2_small_m_large_m_are_bit_identical():
    """"identical MFMA sequence and split-K partition, so identical results" (k_gemm_x3's header)
    and "the same values, bit-identical" (pre-split A): the rows every form can be steered to."""
    c = case(*LARGE[1])
    big, big_ps = large_result(1, False), large_result(1, True)
    assert np.array_equal(big, big_ps)
    x2 = launch(c, "x2", rows=600)                       # 10 x 61 tiles, M > 512
    assert np.array_equal(x2, big[:600])
    for ns in (2, 3, 4):
        sm = launch(c, f"small_m{ns}", rows=512, small_ns=ns)
        assert np.array_equal(sm, big[:512]), ns


def test_split_w_rows_do_not_depend_on_m():
    c = case(70, 130, 768, "w16")
    full = launch(c, "split_w")
    for i in (0, 37, 69):
        ci = c.with_A(c.A_all[i:], M=1)
        assert np.array_equal(launch(ci, "split_w")[0], full[i]), i


# ------------------------------------------------------------------ epilogues
EPI_FORMS = [("generic_f32", (37, 70, 96, "f32"), {}), ("small_m4", (37, 70, 128, "f16"), {}),
             ("x2", (513, 64, 384, "f16"), {}), ("split_w", (70, 130, 128, "w16"), {}),
             ("large_m", (1000, 4090, 128, "f16"), {})]


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


# large-M shares the epilogue code of the others: two modes of it keep the suite quick
EPI_CASES = [(f, s, o, m) for f, s, o in EPI_FORMS for m in ("store", "relu", "resid", "gelu", "mish")
             if f != "large_m" or m in ("store", "gelu")]


@pytest.mark.parametrize("form,shape,opts,mode", EPI_CASES, ids=[f"{e[0]}-{e[3]}" for e in EPI_CASES])
def test_epilogue(form, shape, opts, mode):
    """v = bias + C64 through each epilogue's fp64 formula.  The tolerance on v is the bar times S
    plus one ulp for the bias add; relu is 1-Lipschitz; res + v adds one rounding; gelu and mish
    carry it with a Lipschitz factor of 1.2 plus 4 ulp of the result."""
    c = case(*shape)
    rng = np.random.default_rng(3)
    bias = rng.standard_normal(c.N).astype(np.float32)
    v = c.C64 + bias.astype(np.float64)[None, :]
    tv = c.bar * c.S + ULP * np.abs(v)
    f = dict(opts, bias=bias)
    if mode == "store":
        ref, tol = v, tv
    elif mode == "relu":
        ref, tol = np.maximum(v, 0), tv
    elif mode == "resid":
        res = rng.standard_normal((c.M, c.N + 3)).astype(np.float32)
        f.update(res=res, ldr=c.N + 3)
        ref = res[:, :c.N].astype(np.float64) + v
        tol = tv + ULP * np.abs(ref)
    elif mode == "gelu":
        ref = 0.5 * v * (1.0 + _erf(v / np.sqrt(2.0)))
        tol = 1.2 * tv + 4 * ULP * np.abs(ref)
    else:
        ref = v * np.tanh(np.logaddexp(0.0, v))
        tol = 1.2 * tv + 4 * ULP * np.abs(ref)
    out = launch(c, form, mode, **f)
    worst = float(np.max(np.abs(out - ref) / tol))
    print(f"EPI {form} {mode}: worst |err| / tol {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("kind,form", [("f32", "generic_f32"), ("f16", "generic_f16")])
def test_vqdist_and_argmin(kind, form):
    """(rowsq - 2 h.c) + colsq on the exact-f32 kernel (fp16 weights too: the form stays generic), with
    one planted nearest code per row that argmin_dist_rows must return."""
    from genie_tts_amd.engine import debug_rows
    M, N, K = 37, 256, 128
    c = case(M, N, K, kind, seed=9)
    rng = np.random.default_rng(9)
    planted_all = rng.integers(0, N, O.REF_M)
    planted = planted_all[:M]
    cc = c.with_A(c.W[planted_all] + (rng.standard_normal((O.REF_M, K)) * 0.02 / np.sqrt(K)).astype(np.float32))
    rowsq = (cc.A.astype(np.float64) ** 2).sum(1).astype(np.float32)
    colsq = (c.W.astype(np.float64) ** 2).sum(1).astype(np.float32)
    ref = (rowsq.astype(np.float64)[:, None] - 2 * cc.C64) + colsq.astype(np.float64)[None, :]
    tol = 2 * cc.bar * cc.S + ULP * (np.abs(rowsq[:, None] - 2 * cc.C64) + np.abs(ref))
    # the planted code wins in fp64 by more than the distance tolerance
    order = np.argsort(ref, axis=1)
    assert np.array_equal(order[:, 0], planted)
    gap = ref[np.arange(M), order[:, 1]] - ref[np.arange(M), planted]
    assert np.all(gap > 2 * tol.max())
    out = launch(cc, form, "vqdist", ldc=N, rowsq=rowsq, colsq=colsq)
    assert np.all(np.abs(out - ref) <= tol), float(np.max(np.abs(out - ref) / tol))
    dist = _dev(out)
    idx = torch.full((M,), -1, dtype=torch.int64, device="cuda")
    debug_rows("argmin_dist_rows", M, N, dist, idx)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), planted)


@pytest.mark.parametrize("form,shape,f", [("small_m4", (37, 130, 256), {}), ("x2", (513, 64, 384), {}),
                                          ("large_m", LARGE[0], {})], ids=["small_m4", "x2", "large_m"])
def test_relu_split_planes_are_the_split_of_relu(form, shape, f):
    c = case(*shape)
    bias = np.random.default_rng(4).standard_normal(c.N).astype(np.float32)
    relu = launch(c, form, "relu", bias=bias, **f)
    hi, lo = launch(c, form, "relu_split", bias=bias, **f)
    ehi, elo = O.split_a(relu)
    assert np.array_equal(hi, ehi.astype(np.float32)) and np.array_equal(lo, elo.astype(np.float32))


def _qkv(c, form, M, tmax, nseq, gap, **kv):
    from genie_tts_amd.engine import debug_gemm
    K, ld = c.K, c.K + 8
    A, W = _dev(_padded(c.A[:M], 3, ld)), _dev(_padded(c.w_hi, 3, ld))
    bias = _dev(np.random.default_rng(2).standard_normal(1536).astype(np.float32))
    q = torch.full((M + 2, 517), SENT, device="cuda")
    stride = 16 * tmax * 32 + gap
    kc, vc = (torch.full((nseq * stride,), SENT, device="cuda") for _ in range(2))
    kv = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kv.items()}
    got = debug_gemm(M, 1536, K, a=A, lda=ld, w=W, ldw=ld, bias=bias, c=q, ldc=517, mode="qkv", kv_k=kc, kv_v=vc,
                     kv_tmax=tmax, kv_seq_stride=stride, **kv)
    st = torch.full((M + 2, 1536 + 5), SENT, device="cuda")
    got2 = debug_gemm(M, 1536, K, a=A, lda=ld, w=W, ldw=ld, bias=bias, c=st, ldc=1541, mode="store")
    torch.cuda.synchronize()
    assert got == form and got2 == form
    return q.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy(), st.cpu().numpy()[:M, :1536], stride


@pytest.mark.parametrize("form,M,K,tmax", [("small_m4", 37, 128, 64), ("x2", 513, 128, 600)])
def test_qkv_scatter_pos0(form, M, K, tmax):
    c = case(M, 1536, K)
    pos0 = 5
    q, kc, vc, st, stride = _qkv(c, form, M, tmax, 1, 64, kv_pos0=pos0)
    assert np.array_equal(q[:M, :512], st[:, :512]) and np.all(q[M:] == SENT) and np.all(q[:, 512:] == SENT)
    for cache, col0 in ((kc, 512), (vc, 1024)):
        exp = np.full(stride, SENT, np.float32)
        body = exp[:16 * tmax * 32].reshape(16, tmax, 32)
        body[:, pos0:pos0 + M, :] = st[:, col0:col0 + 512].reshape(M, 16, 32).transpose(1, 0, 2)
        assert np.array_equal(cache, exp)


def test_qkv_scatter_rows_sequences_and_skip():
    M, K, tmax, nseq = 37, 128, 64, 3
    c = case(M, 1536, K)
    rng = np.random.default_rng(6)
    row_seq = (np.arange(M) % nseq).astype(np.int32)
    row_pos = np.zeros(M, np.int32)
    for s in range(nseq):
        n = int((row_seq == s).sum())
        row_pos[row_seq == s] = rng.permutation(tmax)[:n]
    skip = np.array([0, 0, 1], np.uint8)               # sequence 2 is done: it writes nothing
    q, kc, vc, st, stride = _qkv(c, "small_m4", M, tmax, nseq, 96, kv_row_pos=row_pos, kv_row_seq=row_seq,
                                 kv_row_skip=skip)
    assert np.array_equal(q[:M, :512], st[:, :512])
    for cache, col0 in ((kc, 512), (vc, 1024)):
        exp = np.full(nseq * stride, SENT, np.float32)
        for m in range(M):
            s = row_seq[m]
            if skip[s]:
                continue
            body = exp[s * stride:s * stride + 16 * tmax * 32].reshape(16, tmax, 32)
            body[:, row_pos[m], :] = st[m, col0:col0 + 512].reshape(16, 32)
        assert np.array_equal(cache, exp)
        assert np.all(cache[2 * stride:] == SENT)


# ------------------------------------------------------------------ split-K into slabs
def _slices(K, nz):
    steps = K // 128
    return [(128 * (z * steps // nz), 128 * ((z + 1) * steps // nz)) for z in range(nz)]


@pytest.mark.parametrize("form,M,N,kind,f", [("small_m4", 37, 130, "f16", {}), ("small_m2", 37, 130, "f16", {"small_ns": 2}),
                                             ("x2", 513, 64, "f16", {}), ("split_w", 70, 130, "w16", {})],
                         ids=["small_m4", "small_m2", "x2", "split_w"])
@pytest.mark.parametrize("K,nz", [(768, 3), (640, 4), (128, 4)])
def test_split_k_slabs(form, M, N, kind, f, K, nz):
    c = case(M, N, K, kind)
    slabs = launch(c, form, "slab", ksplit=nz, **f)
    check_rho(c, slabs.astype(np.float64).sum(0), f"{form} slabs z={nz}")
    for z, (k0, k1) in enumerate(_slices(K, nz)):
        if k0 == k1:
            assert np.all(slabs[z] == 0), z               # an empty slice writes zeros
        else:
            assert np.array_equal(slabs[z], launch(c, form, "store", k0=k0, k1=k1, **f)), z


# ------------------------------------------------------------------ small activations
@pytest.mark.parametrize("form,shape,f", [("small_m4", (64, 130, 128, "f16"), {}), ("x2", (513, 64, 384, "f16"), {}),
                                          ("large_m", (1000, 4090, 128, "f16"), {}),
                                          ("split_w", (70, 130, 128, "w16"), {})],
                         ids=["small_m4", "x2", "large_m", "split_w"])
def test_small_activations_follow_the_stated_split(form, shape, f):
    """A ~ 1e-3 N(0,1): the lo term of the unscaled split is an fp16 subnormal.  The kernel must
    do its stated arithmetic (subnormal lo terms kept): its distance to the emulated split is
    held to the bar.  Its distance to the true product is printed (tests/NUMERICS.md), not asserted."""
    M, N, K, kind = shape
    c = case(M, N, K, kind, seed=21, scale=1e-3)
    out = launch(c, form, **f)
    r_emu = O.rho(out, c.emulated(), c.S)
    r_flush = O.rho(out, c.emulated(flush_a_lo=True), c.S)
    print(f"SMALLACT {form} K={K}: to emulated split {r_emu:.3g}, to the flushed split {r_flush:.3g}, "
          f"to C64 {c.rho(out):.3g} (emulated split to C64 {c.rho(c.emulated()):.3g}), bar {c.bar:.3g}")
    assert r_emu <= c.bar
