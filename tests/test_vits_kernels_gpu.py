"""GPU: every vocoder kernel of csrc/vits*.hip launched alone through the engine-free hooks
(gsv_debug_conv, gsv_debug_mrf_pair, gsv_debug_mha, gsv_debug_vits_rows) and held to a bar that
comes from an fp64 / fp32 CPU reference (tests/conv_oracle.py, tests/NUMERICS.md).  Every buffer a
kernel writes sits between sentinel-filled margins that must stay untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import conv_oracle as O
from tests import gemm_oracle as G

pytestmark = pytest.mark.gpu

SENT = 777.25            # the sentinel of margins and of never-written elements
MARGIN = 64              # floats on both sides (256 B: the 16-B alignment of the buffer is kept)
SPLIT = 13               # CV_SPLIT_RESID's row split, no multiple of 4


def E():
    from genie_tts_amd import engine
    return engine


class Guard:
    """A device buffer of n elements between two sentinel margins."""

    def __init__(self, n, init=None, dtype=torch.float32, fill=SENT):
        self.buf = torch.full((n + 2 * MARGIN,), fill, dtype=dtype, device="cuda")
        self.t = self.buf[MARGIN:MARGIN + n]
        self.fill = fill
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    def np(self, shape=None):
        torch.cuda.synchronize()
        m = self.buf.cpu().numpy()
        assert np.all(m[:MARGIN] == self.fill) and np.all(m[-MARGIN:] == self.fill), "a margin was written"
        a = m[MARGIN:-MARGIN]
        return a.reshape(shape) if shape is not None else a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def within(got, ref, tol, what, live=None):
    """|got - ref| <= tol on the live columns, exact zeros on the others; returns the worst error / tol."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    if live is not None:
        assert np.all(got[:, ~live] == 0), f"{what}: a gap column is not zero"
        err, tol = err[:, live], tol[:, live]
    assert np.all(np.isfinite(got)), what
    q = float(np.max(err / tol)) if err.size else 0.0
    assert q <= 1.0, f"{what}: error {q:.3g} x its tolerance"
    return q


@functools.lru_cache(maxsize=None)
def case(Cin, Cout, K, Tin, dil=1, kind="f32", in_act=True, pad=None, n_t=None, x_scale=1.0, seed=0):
    """A cached ConvCase; n_t defaults to Tin (an even K then pads one column more on the right)."""
    return O.ConvCase(Cin, Cout, K, Tin, dil=dil, pad=pad, n_t=Tin if n_t is None else n_t, kind=kind, in_act=in_act, x_scale=x_scale, seed=seed)


def aux(c, nseg=2):
    """The epilogues' other operands of a case, fixed by its shape."""
    rng = np.random.default_rng([7, c.Cout, c.n_t])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(res=f(c.Cout, c.n_t), acc=f(c.Cout, c.n_t), vec=f(nseg, c.Cout), res2=f(max(c.Cout - SPLIT, 1), c.n_t))


def two_utterances(n, gap):
    """seg of n columns: utterance 0, `gap` gap columns, utterance 1, one trailing gap column."""
    a = (n - gap - 1) // 2
    seg = np.full(n, -1, np.int32)
    seg[:a] = 0
    seg[a + gap:n - 1] = 1
    return seg


def run_conv(c, mode="store", seg=None, x_tm=False, o_tm=False, w_off=False, part=None, deferred=False, **f):
    """One conv1d launch of a ConvCase through gsv_debug_conv, every written buffer guarded.  Returns the
    form and the buffers as (Cout, n_t) arrays (never-written elements hold SENT)."""
    a = aux(c)
    n = c.Cout * c.n_t
    d = dict(Cin=c.Cin, Tin=c.Tin, Cout=c.Cout, K=c.K, dil=c.dil, pad=c.pad, n_t=c.n_t, o_len=c.n_t,
             in_act=int(c.in_act), in_slope=c.slope, mode=mode, div=3.0, split=SPLIT)
    x = dev(c.x.T if x_tm else c.x)
    d.update(x=x, x_cs=1 if x_tm else c.Tin, x_ts=c.Cin if x_tm else 1)
    if c.kind == "f16":
        ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
        d.update(wh=dev(c.wh()), wscale=dev(c.scale), ovf=ovf)
    else:
        wbuf = torch.zeros(c.w.size + 1, device="cuda")
        w = wbuf[1:] if w_off else wbuf[:-1]
        w.copy_(dev(c.w.reshape(-1)))
        d.update(w=w)
        ovf = None
    if c.bias is not None:
        d.update(bias=dev(c.bias))
    acc0 = (a["acc"].T if o_tm else a["acc"]) if mode in ("acc_add", "acc_mean") else None
    out, acc, out2 = Guard(n), Guard(n, acc0), Guard(a["res2"].size)
    d.update(out=out.t, o_cs=1 if o_tm else c.n_t, o_ts=c.Cout if o_tm else 1)
    if mode in ("resid", "sub", "acc_first", "acc_add", "acc_mean", "resid_vec", "split_resid"):
        d.update(res=dev(a["res"].T if o_tm else a["res"]), r_cs=d["o_cs"], r_ts=d["o_ts"])
    if mode in ("vec", "resid_vec"):
        d.update(vec=dev(a["vec"]), vec_sstride=c.Cout)
    if mode in ("acc_first", "acc_add", "acc_mean"):
        d.update(acc=acc.t)
    if mode == "split_resid":
        d.update(out2=out2.t, res2=dev(a["res2"]))
    if seg is not None:
        d.update(seg=dev(seg))
    if part is not None:
        d.update(part=part.t if isinstance(part, Guard) else part)
    d.update(f)
    form = E().debug_conv(deferred=int(deferred), **d)
    shape = (c.n_t, c.Cout) if o_tm else (c.Cout, c.n_t)
    fix = (lambda m: m.T) if o_tm else (lambda m: m)
    res = {"form": form, "out": fix(out.np(shape)), "acc": fix(acc.np(shape)), "out2": out2.np(a["res2"].shape)}
    if ovf is not None:
        res["ovf"] = int(ovf.item())
    return res


def check_mode(c, mode, got, seg=None, what=""):
    """The buffers of one launch against the fp64 epilogue of the fp64 conv; what the mode does not write
    must hold what it held."""
    a = aux(c)
    vec = a["vec"][np.maximum(seg, 0)].T if seg is not None else a["vec"][0]
    exp = O.epilogue(mode, c.v64, c.tol, res=a["res"], vec=vec, acc=a["acc"], div=3.0, split=SPLIT, res2=a["res2"])
    live = None if seg is None else seg >= 0
    worst = 0.0
    for name, (ref, tol) in exp.items():
        g = got[name][:SPLIT] if (mode, name) == ("split_resid", "out") else got[name]
        worst = max(worst, within(g, ref, tol, f"{what} {mode} {name}", live))
    if "out" not in exp:
        assert np.all(got["out"] == SENT), f"{what} {mode}: out written"
    if "out2" not in exp:
        assert np.all(got["out2"] == SENT), f"{what} {mode}: out2 written"
    if "acc" not in exp:
        assert np.array_equal(got["acc"], a["acc"] if mode == "acc_mean" else np.full_like(a["acc"], SENT)), \
            f"{what} {mode}: acc written"
    if mode == "split_resid":
        assert np.all(got["out"][SPLIT:] == SENT), "rows past split belong to out2"
    return worst


# ------------------------------------------------------------------ f32 k_conv1d
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 7, 11])
@pytest.mark.parametrize("Cin,Cout", [(3, 1), (20, 65), (64, 64)])
def test_f32_conv(K, Cin, Cout):
    """A chunk tail (Cin 3, 20), a row tail (Cout 1, 65), V4 off where Cin K % 4 != 0; one column, one short
    of a tile and one past it, every dilation."""
    worst = 0.0
    for T, dil in ((1, 1), (63, 3), (65, 5)):
        c = case(Cin, Cout, K, T, dil)
        r = run_conv(c)
        assert r["form"] == {"path": "f32", "nsplit": 1, "v4": (Cin * K) % 4 == 0, "slabs": 0}
        worst = max(worst, check_mode(c, "store", r, what=f"f32 K{K} {Cin}->{Cout} T{T} d{dil}"))
        print(f"RHO f32 K={K} {Cin}->{Cout} T={T} dil={dil}: rho {c.rho(r['out']):.3g} bar {c.bar:.3g}")
    print(f"f32 K={K} {Cin}->{Cout}: worst error {worst:.3g} of its tolerance")


def test_f32_conv_layouts():
    """A weight pointer 4 bytes off 16 (the unaligned-weights form), Tin != n_t, time-major input and output."""
    c = case(20, 65, 4, 65, 1)
    r = run_conv(c, w_off=True)
    assert r["form"]["v4"] is False
    check_mode(c, "store", r, what="w + 4 B")
    assert np.array_equal(r["out"], run_conv(c)["out"])          # the float4 form loads the same values
    for pad, n_t in ((0, 60), (7, 70), (2, 10)):
        c2 = case(20, 65, 5, 64, 1, pad=pad, n_t=n_t)
        check_mode(c2, "resid", run_conv(c2, "resid"), what=f"pad {pad} n_t {n_t}")
    c3 = case(20, 65, 3, 65, 3)
    check_mode(c3, "store", run_conv(c3, x_tm=True), what="time-major x")
    check_mode(c3, "resid", run_conv(c3, "resid", o_tm=True), what="time-major out")
    check_mode(c3, "acc_add", run_conv(c3, "acc_add", o_tm=True, x_tm=True), what="time-major both")


# ------------------------------------------------------------------ split-K
def slab_sum(slabs):
    """k_conv_reduce's sum: fp32, in slab order from slab 0."""
    v = slabs[0].copy()
    for z in range(1, slabs.shape[0]):
        v = (v + slabs[z]).astype(np.float32)
    return v


@pytest.mark.parametrize("Cin,Cout,K,T,cap,nsplit", [(192, 384, 5, 37, None, 24), (32, 40, 3, 37, None, 2),
                                                      (192, 384, 5, 37, 9, 9), (192, 384, 5, 37, 3, 3)])
def test_splitk(Cin, Cout, K, T, cap, nsplit):
    """Three groups of 8 slabs, two slabs, part_cap cutting nsplit; the reduce is the in-order fp32 sum of
    the deferred launch's slabs plus the epilogue, bit for bit."""
    c = case(Cin, Cout, K, T, 1, in_act=False)
    n = Cout * T
    cap_n = (cap if cap is not None else nsplit) * n + (n - 1 if cap is not None else 0)
    part = Guard(cap_n)
    r = run_conv(c, "resid", part=part)
    assert r["form"] == {"path": "f32_splitk", "nsplit": nsplit, "v4": True, "slabs": 0}
    check_mode(c, "resid", r, what=f"split-K {nsplit}")
    print(f"RHO split-K {Cin}->{Cout} K={K} nsplit={nsplit}: rho {c.rho(run_conv(c, part=part)['out']):.3g} bar {c.bar:.3g}")
    part2 = Guard(cap_n)
    d = run_conv(c, "resid", part=part2, deferred=True)
    assert d["form"]["slabs"] == nsplit and np.all(d["out"] == SENT)
    slabs = part2.np()[:nsplit * n].reshape(nsplit, Cout, T)
    assert np.all(part2.np()[nsplit * n:] == SENT)
    v = (c.bias[:, None] + slab_sum(slabs)).astype(np.float32)
    assert np.array_equal(r["out"], (aux(c)["res"] + v).astype(np.float32))
    # a segmented reduce: gap columns zero, the live ones unchanged
    seg = two_utterances(T, 3)
    rs = run_conv(c, "resid", part=Guard(cap_n), seg=seg)
    check_mode(c, "resid", rs, seg=seg, what="split-K seg")
    assert np.array_equal(rs["out"][:, seg >= 0], r["out"][:, seg >= 0])


@pytest.mark.parametrize("nsplit_cap", [None, 9, 2])
def test_slab_consumers_equal_reduce_then_consumer(nsplit_cap):
    """ln_channels_slabs and wn_gate_slabs on the slabs of conv1d_deferred are bit-equal to the conv's reduce
    followed by ln_channels / wn_gate (with seg: zeros in the gaps), as their comments claim."""
    Cin, C, K, T = 192, 192, 3, 37
    c = case(Cin, C, K, T, 1, in_act=False)
    n = C * T
    ns = 12 if nsplit_cap is None else nsplit_cap
    rng = np.random.default_rng(3)
    x = dev(rng.standard_normal((C, T)).astype(np.float32))
    g, b = dev((1 + 0.1 * rng.standard_normal(C)).astype(np.float32)), dev((0.1 * rng.standard_normal(C)).astype(np.float32))
    vec = rng.standard_normal((2, C)).astype(np.float32)
    for seg in (None, two_utterances(T, 4)):
        part = Guard(ns * n)
        d = run_conv(c, "store", part=part, deferred=True)
        assert d["form"]["slabs"] == ns
        segd = None if seg is None else dev(seg)
        # LayerNorm: reduce (CV_STORE with bias) then ln_channels(x, y)
        y = run_conv(c, "store", part=Guard(ns * n))["out"]
        o1, o2 = Guard(n), Guard(n)
        E().debug_vits_rows("ln_channels", C=C, T=T, x=x, y=dev(y), out=o1.t, g=g, b=b, seg=segd)
        E().debug_vits_rows("ln_channels_slabs", C=C, T=T, nsplit=ns, x=x, y=part.t, bias=dev(c.bias), out=o2.t, g=g, b=b,
                            seg=segd)
        assert np.array_equal(o1.np(), o2.np())
        if seg is not None:
            assert np.all(o2.np((C, T))[:, seg < 0] == 0) and np.all(o2.np((C, T))[:, seg >= 0] != 0)
        # gate: reduce with CV_VEC (per segment) then wn_gate
        H = C // 2
        xin = run_conv(c, "vec", part=Guard(ns * n), seg=seg, vec=dev(vec))["out"]
        a1, a2 = Guard(H * T), Guard(H * T)
        E().debug_vits_rows("wn_gate", C=H, T=T, x=dev(xin), out=a1.t)
        E().debug_vits_rows("wn_gate_slabs", C=H, T=T, nsplit=ns, x=part.t, bias=dev(c.bias), vec=dev(vec), vec_sstride=C,
                            seg=segd, out=a2.t)
        assert np.array_equal(a1.np(), a2.np())
        ref = np.tanh(xin[:H].astype(np.float64)) / (1 + np.exp(-xin[H:].astype(np.float64)))
        assert np.max(np.abs(a2.np((H, T)) - ref)) <= 4 * 2.0 ** -23          # tanhf, expf and two roundings
        if seg is not None:
            assert np.all(a2.np((H, T))[:, seg < 0] == 0)
        # without a bias
        o3, o4 = Guard(n), Guard(n)
        ysum = slab_sum(part.np()[:ns * n].reshape(ns, C, T))
        E().debug_vits_rows("ln_channels", C=C, T=T, x=x, y=dev(ysum), out=o3.t, g=g, b=b, seg=segd)
        E().debug_vits_rows("ln_channels_slabs", C=C, T=T, nsplit=ns, x=x, y=part.t, out=o4.t, g=g, b=b, seg=segd)
        assert np.array_equal(o3.np(), o4.np())


# ------------------------------------------------------------------ the 11 modes
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_modes(mode, kind):
    """Every ConvMode on Cout = 40 (the FULL and the partial 16-row epilogue both run), plain and with seg
    holding two utterances and a gap."""
    c = case(32 if kind == "f16" else 20, 40, 3, 70, 1, kind=kind)
    tiles = (0, 1, 4) if kind == "f16" else (0,)
    for tf in tiles:
        q = check_mode(c, mode, run_conv(c, mode, tile_force=tf), what=f"{kind} tile {tf}")
        seg = two_utterances(70, 5)
        qs = check_mode(c, mode, run_conv(c, mode, seg=seg, tile_force=tf), seg=seg, what=f"{kind} tile {tf} seg")
        print(f"{kind} {mode} tile_force {tf}: {q:.3g} / {qs:.3g} of the tolerance")


# ------------------------------------------------------------------ k_conv_h
@pytest.mark.parametrize("K", [1, 2, 3, 4, 7, 11])
@pytest.mark.parametrize("Cin", [32, 64, 24, 48])
def test_conv_h(K, Cin):
    """Every tap count x channel chunk (32: Cin 32 / 64; 8: Cin 24 / 48) x tile; Cout 16 / 24 / 40; one
    column, a full tile, one past it and 257 columns; every dilation."""
    worst = 0.0
    for i, (T, dil) in enumerate(((1, 1), (64, 3), (65, 5), (257, 1))):
        Cout = (16, 24, 40, 24)[i]
        c = case(Cin, Cout, K, T, dil, kind="f16")
        for tf in (1, 2, 3, 4):
            r = run_conv(c, tile_force=tf)
            assert r["form"] == {"path": "conv_h", "chunk": 32 if Cin % 32 == 0 else 8, "tile": tf - 1, "slabs": 0}
            assert r["ovf"] == 0
            check_mode(c, "store", r, what=f"conv_h K{K} Cin{Cin} Cout{Cout} T{T} d{dil} tile{tf}")
            rho = c.rho(r["out"])
            worst = max(worst, rho / c.bar)
            if tf == 1 or T == 257:
                print(f"RHO conv_h K={K} Cin={Cin} Cout={Cout} T={T} dil={dil} tile={tf - 1}: rho {rho:.3g} bar {c.bar:.3g}")
    print(f"conv_h K={K} Cin={Cin}: worst rho / bar {worst:.3g}")


@pytest.mark.parametrize("tf", [1, 2, 3, 4])
@pytest.mark.parametrize("K,Cin,dil", [(7, 32, 3), (3, 24, 5), (11, 64, 1)])
def test_conv_h_segments_equal_single_launches(tf, K, Cin, dil):
    """Two utterances back to back with a zero gap and seg: each utterance's columns are bit-equal to the
    launch on that utterance alone (an output's accumulation order is (chunk, tap, group), whatever its
    column), and the gap is zero."""
    Cout, T1, T2 = 24, 70, 61
    pad = dil * (K - 1) // 2
    gap = pad + 2
    c1 = case(Cin, Cout, K, T1, dil, kind="f16", seed=1)
    c2 = O.ConvCase(Cin, Cout, K, T2, dil=dil, kind="f16", in_act=True, seed=1)
    c2.w, c2.scale, c2.bias = c1.w, c1.scale, c1.bias             # one conv, two inputs
    T = T1 + gap + T2
    x = np.zeros((Cin, T), np.float32)
    x[:, :T1], x[:, T1 + gap:] = c1.x, c2.x
    cb = O.ConvCase(Cin, Cout, K, T, dil=dil, kind="f16", in_act=True, seed=1, x=x)
    cb.w, cb.scale, cb.bias = c1.w, c1.scale, c1.bias
    seg = np.full(T, -1, np.int32)
    seg[:T1], seg[T1 + gap:] = 0, 1
    both = run_conv(cb, seg=seg, tile_force=tf)["out"]
    assert np.array_equal(both[:, :T1], run_conv(c1, tile_force=tf)["out"])
    assert np.array_equal(both[:, T1 + gap:], run_conv(c2, tile_force=tf)["out"])
    assert np.all(both[:, T1:T1 + gap] == 0)
    within(both[:, :T1], c1.v64, c1.tol, "utterance 0 against fp64")


# ------------------------------------------------------------------ polyphase ConvTranspose
@pytest.mark.parametrize("u,k", [(10, 16), (8, 16), (2, 8), (2, 2), (10, 20)])
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_polyphase(u, k, kind):
    """ConvTranspose1d(32 -> 16, k, stride u, pad (k - u) / 2) as u polyphase convs with the engine's geometry
    (pad M - 1, o_tstride u, o_toff -(k - u) / 2, o_len clipping the last phases), against torch's fp64
    conv_transpose1d on the unfolded weight; on the f16 path with the weight norm as in_scale and every tile."""
    Cin, Cout = 32, 16
    M, padT = (k + u - 1) // u, (k - u) // 2
    rng = np.random.default_rng([u, k])
    v_all = (rng.standard_normal((Cin, G.REF_N, k)) / np.sqrt(Cin * M)).astype(np.float32)
    if kind == "f16":
        v_all = G.f16(v_all).astype(np.float32)
    isc = (rng.random(Cin) + 0.5).astype(np.float32) if kind == "f16" else None
    bias = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    v = np.ascontiguousarray(v_all[:, :Cout])
    W = O.polyphase(v, u)                                              # (u, Cout, Cin, M)
    # the bar: rho_seq on 64 im2col rows x 256 weight rows of phase 0 of the same operands
    x_all = rng.standard_normal((Cin, G.REF_M + M)).astype(np.float32)
    a_ref = O.im2col(x_all, M, 1, M - 1, G.REF_M, True, 0.1, isc)
    w_ref = O.polyphase(v_all, u)[0].reshape(G.REF_N, Cin * M)
    bar = G.MARGIN * G.rho(G.gemm_f32_seq(a_ref, w_ref), *G.exact(a_ref, w_ref))
    for Tin in (1, 5, 33):
        x = np.ascontiguousarray(x_all[:, :Tin])
        Tn = (Tin - 1) * u - 2 * padT + k
        xa = O.lrelu32(x, 0.1).astype(np.float64) * (isc.astype(np.float64)[:, None] if isc is not None else 1.0)
        ref = O.conv_transpose64(xa, v, u, padT) + bias.astype(np.float64)[:, None]
        S = O.conv_transpose64(np.abs(xa), np.abs(v), u, padT)
        tol = (bar + (O.EPS if isc is not None else 0.0)) * S + O.EPS * np.abs(ref)     # in_scale: one fp32 multiply
        assert ref.shape == (Cout, Tn)
        o_cs = Tn + 3                                                   # three columns past o_len per row
        d = dict(Cin=Cin, Tin=Tin, Cout=Cout, K=M, dil=1, pad=M - 1, n_t=(Tn + padT + u - 1) // u, o_tstride=u,
                 o_toff=-padT, o_len=Tn, in_act=1, in_slope=0.1, phases=u, x=dev(x), x_cs=Tin, bias=dev(bias), o_cs=o_cs)
        if kind == "f16":
            wh = dev(G.f16(W).transpose(0, 1, 3, 2))                    # [phase][Cout][M][Cin]
            ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
            d.update(wh=wh, wh_phase_stride=Cout * M * Cin, wscale=dev(np.ones(Cout, np.float32)), ovf=ovf, in_scale=dev(isc))
        else:
            d.update(w=dev(W), w_phase_stride=Cout * Cin * M)
        q = 0.0
        for tf in ((1, 2, 3, 4) if kind == "f16" else (0,)):
            out = Guard(Cout * o_cs)
            form = E().debug_conv(out=out.t, tile_force=tf, **d)
            assert form["path"] == ("conv_h" if kind == "f16" else "f32")
            got = out.np((Cout, o_cs))
            assert np.all(got[:, Tn:] == SENT), "a column at or past o_len was written"
            q = max(q, within(got[:, :Tn], ref, tol, f"polyphase {kind} u{u} k{k} Tin{Tin} tile{tf}"))
        print(f"RHO polyphase {kind} u={u} k={k} Tin={Tin}: {q:.3g} of its tolerance, bar {bar:.3g}")


# ------------------------------------------------------------------ k_conv_ws
@pytest.mark.parametrize("C,K", [(64, 7), (64, 11), (128, 7)])
def test_conv_ws(C, K):
    """The weight-stationary form (ws = 8 CUs, tile 0, 4099 columns: 17 tiles over 8 lanes) in the five MRF
    modes with seg: within the bar, and bit-identical to k_conv_h's (2, 2, 1) form on the same arguments."""
    T = 4099
    c = case(C, C, K, T, 3, kind="f16")
    seg = np.zeros(T, np.int32)
    seg[2000:2011], seg[2011:], seg[-2:] = -1, 1, -1
    for mode in ("store", "resid", "acc_first", "acc_add", "acc_mean"):
        r = run_conv(c, mode, seg=seg, tile_force=1, ws=8)
        assert r["form"] == {"path": "conv_ws", "chunk": 32, "tile": 0, "slabs": 0} and r["ovf"] == 0
        q = check_mode(c, mode, r, seg=seg, what=f"conv_ws C{C} K{K}")
        h = run_conv(c, mode, seg=seg, tile_force=1, ws=0)
        assert h["form"]["path"] == "conv_h"
        for name in ("out", "acc"):
            assert np.array_equal(r[name], h[name]), (mode, name)
        print(f"conv_ws C={C} K={K} {mode}: {q:.3g} of its tolerance")
    r = run_conv(c, tile_force=1, ws=8)
    print(f"RHO conv_ws C={C} K={K} T={T}: rho {c.rho(r['out']):.3g} bar {c.bar:.3g}")


# ------------------------------------------------------------------ mrf_pair
class MrfCase:
    """One ResBlock step: conv1 (K taps, dilation d) and conv2 (K taps) C -> C on r (C, T), fp16-valued
    weights with scales; the fp64 reference of both convs and the tolerance
    bar2 S2 + |W2| (x) (bar1 S1) (LeakyReLU is 1-Lipschitz), with the roundings of the scales and biases."""

    def __init__(self, K, C, dil, T, seg=None, x_scale=1.0, r=None):
        self.K, self.C, self.dil, self.T, self.seg = K, C, dil, T, seg
        self.c1 = c1 = case(C, C, K, max(T, 1), dil, kind="f16", x_scale=x_scale, seed=2) if r is None else \
            O.ConvCase(C, C, K, T, dil=dil, kind="f16", in_act=True, seed=2, x=r)
        self.c2 = c2 = case(C, C, K, 64, 1, kind="f16", seed=3)           # conv2's weights, scale, bias and bar
        self.r = c1.x
        live = np.ones(T, bool) if seg is None else seg >= 0
        self.live = live
        xt = c1.v64.copy()
        xt = np.where(xt >= 0, xt, 0.1 * xt) * live[None, :]
        self.xt64 = xt
        t1 = c1.tol * live[None, :]
        p2 = (K - 1) // 2
        A2 = O.im2col64(xt, K, 1, p2, T)
        W2 = c2.Wm.astype(np.float64)
        C2, S2 = A2 @ W2.T, np.abs(A2) @ np.abs(W2).T
        sc = c2.scale.astype(np.float64)[:, None]
        self.v64 = (C2.T * sc) + c2.bias.astype(np.float64)[:, None]
        prop = (O.im2col64(t1, K, 1, p2, T) @ np.abs(W2).T).T * np.abs(sc)
        self.tol = c2.bar * S2.T * np.abs(sc) + prop + O.EPS * np.abs(C2.T * sc) + O.EPS * np.abs(self.v64)

    def emulated(self):
        """The kernel's stated arithmetic: both convs as emulated splits, xt rounded to fp32 between them."""
        c1, c2 = self.c1, self.c2
        xt = c1.emulated()
        xt = (np.where(xt >= 0, xt, 0.1 * xt) * self.live[None, :]).astype(np.float32)
        A2 = O.im2col(xt, self.K, 1, (self.K - 1) // 2, self.T)
        C = G.emulated_split(A2, G.f16(c2.Wm)).T * c2.scale.astype(np.float64)[:, None]
        return C + c2.bias.astype(np.float64)[:, None]

    def run(self, mode, r=None):
        c1, c2, T, C = self.c1, self.c2, self.T, self.C
        a = aux(c1)
        n = C * T
        out, acc = Guard(n), Guard(n, a["acc"] if mode in ("acc_add", "acc_mean") else None)
        ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
        f = dict(T=T, C=C, K=self.K, dil=self.dil, r=dev(self.r if r is None else r), w1=dev(c1.wh()), s1=dev(c1.scale),
                 b1=dev(c1.bias), w2=dev(c2.wh()), s2=dev(c2.scale), bias2=dev(c2.bias), ovf=ovf, out=out.t, div=3.0)
        if mode != "resid":
            f.update(acc=acc.t)
        if self.seg is not None:
            f.update(seg=dev(self.seg))
        E().debug_mrf_pair(mode=mode, **f)
        return {"out": out.np((C, T)), "acc": acc.np((C, T)), "ovf": int(ovf.item())}

    def check(self, mode, got, what):
        a = aux(self.c1)
        exp = O.epilogue(mode, self.v64, self.tol, res=self.r, acc=a["acc"], div=3.0)
        live = None if self.seg is None else self.live
        q = 0.0
        for name, (ref, tol) in exp.items():
            q = max(q, within(got[name], ref, tol, f"{what} {mode} {name}", live))
        if "out" not in exp:
            assert np.all(got["out"] == SENT)
        if "acc" not in exp:
            assert np.array_equal(got["acc"], a["acc"] if mode == "acc_mean" else np.full_like(a["acc"], SENT))
        assert got["ovf"] == 0
        return q


MRF_MODES = ("resid", "acc_first", "acc_add", "acc_mean")


@pytest.mark.parametrize("K", [3, 7, 11])
@pytest.mark.parametrize("C", [16, 32])
def test_mrf_pair(K, C):
    """Every instance x dilation x mode; one column, one short of a 224-column step, one past it, two steps and
    a column; seg with gaps (a gap in the middle, a trailing one)."""
    Ts = (1, 223, 225, 449)
    i = 0
    for dil in (1, 3, 5):
        for mode in MRF_MODES:
            T = Ts[i % 4]
            seg = two_utterances(T, 6) if (i // 4) % 2 == 1 and T > 20 else None
            i += 1
            m = MrfCase(K, C, dil, T, seg)
            q = m.check(mode, m.run(mode), f"mrf K{K} C{C} d{dil} T{T}")
            print(f"RHO mrf_pair K={K} C={C} dil={dil} T={T} {mode}{' seg' if seg is not None else ''}: "
                  f"{q:.3g} of its tolerance (bars {m.c1.bar:.3g}, {m.c2.bar:.3g})")
    # seg at every T the loop ran without one
    for T in (223, 449):
        seg = two_utterances(T, 6)
        m = MrfCase(K, C, 3, T, seg)
        m.check("resid", m.run("resid"), f"mrf K{K} C{C} seg T{T}")


def test_mrf_pair_range_guard():
    m = MrfCase(3, 16, 1, 225)
    assert m.run("resid")["ovf"] == 0
    r = m.r.copy()
    r[5, 100] = 1e6                                   # no fp16 hi part
    assert m.run("resid", r=r)["ovf"] == 1


@pytest.mark.parametrize("C,T", [(32, 57600), (16, 115000)])
def test_mrf_pair_persistent_loop(C, T):
    """More steps of 224 columns than blocks (256 per-CU blocks at C = 32, 512 at C = 16): 258 and 514 steps."""
    m = MrfCase(3, C, 3, T)
    q = m.check("resid", m.run("resid"), f"mrf persistent C{C}")
    print(f"RHO mrf_pair persistent C={C} T={T}: {q:.3g} of its tolerance")


# ------------------------------------------------------------------ attention
def run_mha(q, k, v, heads, dk, scale, postdiv=False, ek=None, ev=None, window=0, ranges=None, cm=False):
    """One k_mha launch; cm: channel-major buffers [C][T] (ts 1, cs rows), else time-major [T][C]."""
    nq, nk, Cw = q.shape[0], k.shape[0], heads * dk
    lay = (lambda a: a.T) if cm else (lambda a: a)
    st = lambda n: dict(ts=1, cs=n) if cm else dict(ts=Cw, cs=1)
    out = Guard(nq * Cw)
    f = dict(nq=nq, nk=nk, heads=heads, dk=dk, postdiv=int(postdiv), scale=scale, window=window,
             q=dev(lay(q)), k=dev(lay(k)), v=dev(lay(v)), out=out.t)
    for name, n in (("q", nq), ("k", nk), ("v", nk), ("o", nq)):
        f[f"{name}_ts"], f[f"{name}_cs"] = st(n)["ts"], st(n)["cs"]
    if ek is not None:
        f.update(ek=dev(ek), ev=dev(ev))
    if ranges is not None:
        rs = np.ascontiguousarray(ranges, np.int32)
        f.update(row_seg=dev(rs), row_seg_host=rs)
    E().debug_mha(**f)
    o = out.np((Cw, nq) if cm else (nq, Cw))
    return o.T if cm else o


def mha_check(got, args, kw, what):
    ref = O.mha_ref(*args, **kw)
    bar = 4.0 * float(np.max(np.abs(O.mha_ref(*args, **kw, dtype=np.float32).astype(np.float64) - ref)))
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"RHO mha {what}: error {err:.3g} bar {bar:.3g}")
    assert bar > 0 and err <= bar, (what, err, bar)


def qkv(rng, nq, nk, Cw):
    return tuple(rng.standard_normal((n, Cw)).astype(np.float32) for n in (nq, nk, nk))


@pytest.mark.parametrize("n", [1, 3, 9, 257, 2048])
def test_mha_self_attention_with_relpos(n):
    rng = np.random.default_rng(n)
    q, k, v = qkv(rng, n, n, 192)
    ek, ev = (rng.standard_normal((9, 96)).astype(np.float32) * s for s in (0.1, 0.1))
    kw = dict(ek=ek, ev=ev, window=4)
    sc = float(np.sqrt(96.0))
    for cm in (True, False):
        mha_check(run_mha(q, k, v, 2, 96, sc, cm=cm, **kw), (q, k, v, 2, 96, sc), kw, f"self n={n} cm={cm}")


def test_mha_cross_and_postdiv():
    rng = np.random.default_rng(5)
    q, k, v = qkv(rng, 7, 300, 512)
    sc = float(np.sqrt(128.0))
    for cm in (True, False):
        mha_check(run_mha(q, k, v, 4, 128, sc, cm=cm), (q, k, v, 4, 128, sc), {}, f"cross 7 x 300 cm={cm}")
    q, k, v = qkv(rng, 33, 33, 128)
    for cm in (True, False):
        mha_check(run_mha(q, k, v, 2, 64, sc, postdiv=True, cm=cm), (q, k, v, 2, 64, sc), dict(postdiv=True),
                  f"postdiv cm={cm}")


@pytest.mark.parametrize("cross", [False, True])
def test_mha_row_seg(cross):
    """Three packed sequences of 1, 5 and 260 rows: every row equals the same row of its sequence launched
    alone, bit for bit, and meets the bar."""
    rng = np.random.default_rng(8)
    lens = (1, 5, 260)
    nk = sum(lens)
    qlens = (2, 3, 4) if cross else lens
    q, k, v = qkv(rng, sum(qlens), nk, 192)
    ek, ev = (rng.standard_normal((9, 96)).astype(np.float32) * 0.1 for _ in range(2))
    kw = {} if cross else dict(ek=ek, ev=ev, window=4)
    sc = float(np.sqrt(96.0))
    ranges, k0 = [], 0
    for ql, kl in zip(qlens, lens):
        ranges += [(k0, kl)] * ql
        k0 += kl
    for cm in (True, False):
        got = run_mha(q, k, v, 2, 96, sc, ranges=ranges, cm=cm, **kw)
        mha_check(got, (q, k, v, 2, 96, sc), dict(ranges=ranges, **kw), f"row_seg cross={cross} cm={cm}")
        q0 = k0 = 0
        for ql, kl in zip(qlens, lens):
            alone = run_mha(q[q0:q0 + ql], k[k0:k0 + kl], v[k0:k0 + kl], 2, 96, sc, cm=cm, **kw)
            assert np.array_equal(got[q0:q0 + ql], alone), (cross, cm, kl)
            q0, k0 = q0 + ql, k0 + kl


# ------------------------------------------------------------------ LayerNorm over channels
def ln_columns(C, T, rng):
    """(T, C) rows of NUMERICS.md's three kinds: N(0,1); with T >= 3 a constant 0.75 and 1e3 + N(0,1)."""
    v = rng.standard_normal((T, C)).astype(np.float32)
    if T >= 3:
        v[1] = 0.75
        v[2] += np.float32(1e3)
    return v


def ln_bar(C, rng, g, b):
    """4 x the rho_ln of torch's fp32 layer_norm on 64 rows of the three kinds."""
    v = rng.standard_normal((64, C)).astype(np.float32)
    v[1] = 0.75
    v[2::4] += np.float32(1e3)
    t = torch.nn.functional.layer_norm(torch.from_numpy(v), (C,), torch.from_numpy(g), torch.from_numpy(b), 1e-5)
    return 4.0 * G.ln_rho(t.numpy(), v, g, b, 1e-5)


@pytest.mark.parametrize("C,Ts", [(192, (1, 3, 5)), (100, (1, 63, 65)), (255, (1, 63, 65)), (16, (5,)), (256, (5,))])
def test_ln_channels(C, Ts):
    rng = np.random.default_rng(C)
    g = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    bar = ln_bar(C, rng, g, b)
    for T in Ts:
        v = ln_columns(C, T, rng)
        y = rng.standard_normal((T, C)).astype(np.float32) * (np.abs(v) < 100)       # x + y, y kept off the big rows
        if T >= 3:
            y[1] = 0
        for with_y in (False, True):
            vin = (v + y).astype(np.float32) if with_y else v
            out = Guard(C * T)
            E().debug_vits_rows("ln_channels", C=C, T=T, x=dev(v.T), y=dev(y.T) if with_y else None, out=out.t, g=dev(g),
                                b=dev(b))
            got = out.np((C, T))
            r = O.ln_channels_rho(got, vin.T, g, b)
            print(f"RHO ln_channels C={C} T={T} y={with_y}: rho_ln {r:.3g} bar {bar:.3g}")
            assert r <= bar
            if T >= 3:
                assert np.array_equal(got[:, 1], b)                                     # the constant column
    if C % 16 == 0:
        T = 9
        v = ln_columns(C, T, rng)
        seg = np.int32([0, 0, 0, -1, -1, 1, 1, 1, -1])
        out = Guard(C * T)
        E().debug_vits_rows("ln_channels", C=C, T=T, x=dev(v.T), out=out.t, g=dev(g), b=dev(b), seg=dev(seg))
        got = out.np((C, T))
        assert np.all(got[:, seg < 0] == 0)
        assert O.ln_channels_rho(got[:, seg >= 0], v.T[:, seg >= 0], g, b) <= bar


@pytest.mark.parametrize("nsplit", [2, 8, 9, 24])
def test_ln_channels_slabs(nsplit):
    C, T = 192, 7
    rng = np.random.default_rng(nsplit)
    g = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    bar = ln_bar(C, rng, g, b)
    x = ln_columns(C, T, rng).T.copy()
    slabs = (rng.standard_normal((nsplit, C, T)) / np.sqrt(nsplit)).astype(np.float32)
    slabs[:, :, 1:3] = 0                                   # the constant and the 1e3 columns keep their kind
    bias = (0.1 * rng.standard_normal(C)).astype(np.float32)
    seg = np.int32([0, 0, 0, 0, -1, 1, -1])
    for bv in (None, bias):
        for sg in (None, seg):
            y = slab_sum(slabs)                            # the kernels' order: slabs from 0, then the bias, then x
            if bv is not None:
                y = (bv[:, None] + y).astype(np.float32)
            vin = (x + y).astype(np.float32)
            out = Guard(C * T)
            E().debug_vits_rows("ln_channels_slabs", C=C, T=T, nsplit=nsplit, x=dev(x), y=dev(slabs),
                                bias=None if bv is None else dev(bv), out=out.t, g=dev(g), b=dev(b),
                                seg=None if sg is None else dev(sg))
            got = out.np((C, T))
            live = np.ones(T, bool) if sg is None else sg >= 0
            assert np.all(got[:, ~live] == 0)
            if bv is None:
                assert np.array_equal(got[:, 1], b)        # the constant column
            r = O.ln_channels_rho(got[:, live], vin[:, live], g, b)
            print(f"RHO ln_channels_slabs nsplit={nsplit} bias={bv is not None} seg={sg is not None}: rho_ln {r:.3g} bar {bar:.3g}")
            assert r <= bar


# ------------------------------------------------------------------ mean3, seg_fill
@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_mean3(n):
    rng = np.random.default_rng(n)
    a, b, c = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    ref = (((a + b).astype(np.float32) + c).astype(np.float32) / np.float32(3.0)).astype(np.float32)
    out = Guard(n)
    E().debug_vits_rows("mean3", n=n, div=3.0, x=dev(a), y=dev(b), z=dev(c), out=out.t)
    assert np.array_equal(out.np(), ref)
    # buffers 4 bytes off 16: the scalar kernel alone
    pad = lambda v: torch.cat([torch.zeros(1, device="cuda"), dev(v)])[1:]
    out2 = Guard(n + 1)
    E().debug_vits_rows("mean3", n=n, div=3.0, x=pad(a), y=pad(b), z=pad(c), out=out2.t[1:])
    assert np.array_equal(out2.np()[1:], ref) and out2.np()[0] == SENT


@pytest.mark.parametrize("f", [1, 640])
def test_seg_fill(f):
    off, ln = [0, 3, 5, 9], [3, 2, 2, 1]                 # touching segments, a gap, a trailing gap
    n = 12 * f + 5
    out = Guard(n, dtype=torch.int32, fill=-7)
    E().debug_vits_rows("seg_fill", n=n, nseg=4, f=f, off=dev(np.int32(off)), len=dev(np.int32(ln)), out=out.t)
    assert np.array_equal(out.np(), O.seg_fill_ref(n, off, ln, f))
    one = Guard(5, dtype=torch.int32, fill=-7)
    E().debug_vits_rows("seg_fill", n=5, nseg=1, f=f, off=dev(np.int32([0])), len=dev(np.int32([1])), out=one.t)
    assert np.array_equal(one.np(), O.seg_fill_ref(5, [0], [1], f))


# ------------------------------------------------------------------ small activations
def test_small_activations_follow_the_stated_split():
    """x ~ 1e-3 N(0,1): the lo terms are fp16 subnormals.  The kernels are held to their stated arithmetic
    (the emulated split) within the bar; their distance to the fp64 conv is reported, not asserted."""
    # no bias: beside sums of 1e-3 the rounding of a 0.1 bias add would be all that is measured
    c = O.ConvCase(64, 40, 7, 257, dil=3, kind="f16", in_act=True, x_scale=1e-3, bias=False)
    r = run_conv(c, tile_force=1)
    em = c.emulated()
    q = within(r["out"], em, c.tol, "conv_h small activations to the emulated split")
    flushed = c.emulated(flush_a_lo=True)
    print(f"RHO small conv_h: kernel to emulated split {q:.3g} of the tolerance (bar {c.bar:.3g}); "
          f"rho kernel to fp64 {c.rho(r['out']):.3g}, emulated to fp64 {c.rho(em):.3g}, "
          f"kernel to a flushed-lo split {np.max(np.abs(r['out'] - flushed) / c.tol):.3g} of the tolerance")
    m = MrfCase(7, 32, 3, 225, x_scale=1e-3)
    got = m.run("acc_first")
    exp_em = m.emulated() + m.r.astype(np.float64)
    q = within(got["acc"], exp_em, m.tol + O.EPS * np.abs(exp_em), "mrf_pair small activations to the emulated split")
    ref = m.v64 + m.r.astype(np.float64)
    print(f"RHO small mrf_pair: kernel to emulated split {q:.3g} of the tolerance; kernel to fp64 "
          f"{np.max(np.abs(got['acc'] - ref) / (m.tol + O.EPS * np.abs(ref))):.3g} of the tolerance")
