"""CPU: the conv oracle's own checks, the sharpness of its bar, and the host side of gsv_debug_conv /
gsv_debug_mrf_pair / gsv_debug_mha / gsv_debug_vits_rows (struct layouts, every argument rejection
and the conv dispatch rule conv_form through the dry path; no HIP call)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import conv_oracle as O
from tests import gemm_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY = [(10, 16), (8, 16), (2, 8), (2, 2), (10, 20)]          # (stride u, kernel k) of the ConvTranspose cases


# ------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("Cin,Cout,K,Tin,dil,pad", [(3, 5, 1, 9, 1, 0), (4, 3, 3, 17, 3, 3), (8, 2, 11, 70, 5, 25),
                                                     (5, 4, 5, 20, 1, 0), (6, 3, 7, 30, 2, 9), (2, 2, 4, 12, 1, 2)])
def test_im2col_gemm_is_torch_conv1d(Cin, Cout, K, Tin, dil, pad):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(K)
    x = rng.standard_normal((Cin, Tin)).astype(np.float32)
    w = rng.standard_normal((Cout, Cin, K)).astype(np.float32)
    n_t = Tin + 2 * pad - dil * (K - 1)                      # Tin != n_t wherever 2 pad != dil (K - 1)
    for act in (False, True):
        A = O.im2col(x, K, dil, pad, n_t, in_act=act, slope=0.1)
        got = (A.astype(np.float64) @ w.reshape(Cout, -1).astype(np.float64).T).T
        xa = O.lrelu32(x, 0.1) if act else x
        ref = F.conv1d(torch.from_numpy(xa).double()[None], torch.from_numpy(w).double(), padding=pad, dilation=dil)[0]
        assert got.shape == tuple(ref.shape)
        np.testing.assert_allclose(got, ref.numpy(), rtol=0, atol=1e-12)
    # fewer output columns than the input gives, and an input scale
    s = rng.random(Cin).astype(np.float32) + 0.5
    A = O.im2col(x, K, dil, pad, max(n_t - 3, 1), in_scale=s)
    ref = F.conv1d(torch.from_numpy(x * s[:, None]).double()[None], torch.from_numpy(w).double(), padding=pad,
                   dilation=dil)[0][:, :max(n_t - 3, 1)]
    np.testing.assert_allclose((A.astype(np.float64) @ w.reshape(Cout, -1).astype(np.float64).T).T, ref.numpy(), atol=1e-12)


def poly_full(x, w, u):
    """The unpadded transpose from the polyphase convs: column t u + r = phase r's conv at t."""
    Cin, Cout, k = w.shape
    W = O.polyphase(w, u)
    M = W.shape[3]
    n_t = x.shape[1] + M - 1
    y = np.zeros((Cout, n_t * u))
    for r in range(u):
        A = O.im2col(x, M, 1, M - 1, n_t)
        y[:, r::u] = (A.astype(np.float64) @ W[r].reshape(Cout, -1).astype(np.float64).T).T
    return y


@pytest.mark.parametrize("u,k", POLY)
@pytest.mark.parametrize("Tin", [1, 5, 33])
def test_polyphase_is_torch_conv_transpose1d(u, k, Tin):
    rng = np.random.default_rng(u * 100 + k)
    x = rng.standard_normal((6, Tin)).astype(np.float32)
    w = rng.standard_normal((6, 4, k)).astype(np.float32)
    padT = (k - u) // 2
    ref = O.conv_transpose64(x, w, u, padT)
    full = poly_full(x, w, u)
    np.testing.assert_allclose(full[:, padT:padT + ref.shape[1]], ref, atol=1e-12)
    assert np.all(full[:, padT + ref.shape[1] + padT:] == 0)      # past k - 1 + (Tin - 1) u: the zero taps


FAMILIES = [(32, 1, 1), (24, 2, 1), (48, 3, 3), (64, 4, 1), (32, 7, 5), (64, 11, 1), (16, 3, 1), (32, 11, 5)]


@pytest.mark.parametrize("Cin,K,dil", FAMILIES)
def test_conv_bar_is_sharp(Cin, K, dil):
    """4 rho_seq is at most half the rho of each wrong conv, for the (Cin, K) families of the GPU tests."""
    c = O.ConvCase(Cin, 40, K, 200, dil=dil, seed=5, kind="f16", in_act=True)
    assert c.rho(c.emulated()) <= c.bar / 4
    for name, C in O.wrong_convs(c).items():
        r = G.rho(C, c.C64, c.S)
        print(f"Cin={Cin} K={K}: bar {c.bar:.3g}, {name} {r:.3g}")
        assert c.bar <= 0.5 * r, (name, c.bar, r)


def test_conv_bar_is_sharp_for_swapped_phases():
    rng = np.random.default_rng(9)
    u, k, Cin, Cout, Tin = 2, 8, 32, 16, 33
    x = rng.standard_normal((Cin, Tin)).astype(np.float32)
    w = G.f16(rng.standard_normal((Cin, Cout, k)) / np.sqrt(Cin * k)).astype(np.float32)
    W = O.polyphase(w, u)
    M = W.shape[3]
    n_t = Tin + M - 1
    A = O.im2col(x, M, 1, M - 1, n_t)
    for r in range(u):
        C64, S = G.exact(A, W[r].reshape(Cout, -1))
        a_ref = O.im2col(rng.standard_normal((Cin, 80)).astype(np.float32), M, 1, M - 1, G.REF_M)
        w_ref = G.f16(rng.standard_normal((G.REF_N, Cin * M)) / np.sqrt(Cin * k)).astype(np.float32)
        bar = G.MARGIN * G.rho(G.gemm_f32_seq(a_ref, w_ref), *G.exact(a_ref, w_ref))
        swapped = G.emulated_split(A, G.f16(W[1 - r].reshape(Cout, -1)))
        assert bar <= 0.5 * G.rho(swapped, C64, S)
        assert G.rho(G.emulated_split(A, G.f16(W[r].reshape(Cout, -1))), C64, S) <= bar / 4


def test_epilogue_tolerances_and_tanh():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((4, 7))
    tol = np.full((4, 7), 1e-6)
    res, acc, vec = rng.standard_normal((4, 7)), rng.standard_normal((4, 7)), rng.standard_normal(4)
    o, t = O.epilogue("acc_mean", v, tol, res=res, acc=acc, div=3.0)["out"]
    np.testing.assert_allclose(o, (acc + (res + v)) / 3.0)
    assert np.all(t >= tol / 3) and np.all(t <= tol / 3 + 4 * O.EPS * (np.abs(o) + np.abs(res + v) + np.abs(acc + res + v)))
    d = O.epilogue("split_resid", v, tol, res=res, res2=acc[:1], split=3)
    assert d["out"][0].shape == (3, 7) and d["out2"][0].shape == (1, 7)
    np.testing.assert_allclose(O.epilogue("resid_vec", v, tol, res=res, vec=vec)["out"][0], res + v + vec[:, None])
    assert 0 < O.tanh_err(v) < 4 * O.EPS
    assert set(O.MODES) == set(_lib().CONV_MODES)


def test_mha_reference_matches_a_plain_restatement():
    rng = np.random.default_rng(4)
    q, k, v = (rng.standard_normal((5, 8)).astype(np.float32) for _ in range(3))
    ek, ev = (rng.standard_normal((5, 4)).astype(np.float32) for _ in range(2))
    got = O.mha_ref(q, k, v, 2, 4, 2.0, ek=ek, ev=ev, window=2)
    for h in range(2):
        c = slice(4 * h, 4 * h + 4)
        s = (q[:, c].astype(np.float64) / 2.0) @ k[:, c].astype(np.float64).T
        for i in range(5):
            for j in range(5):
                if abs(j - i) <= 2:
                    s[i, j] += (q[i, c].astype(np.float64) / 2.0) @ ek[j - i + 2]
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        o = p @ v[:, c].astype(np.float64)
        for i in range(5):
            for j in range(5):
                if abs(j - i) <= 2:
                    o[i] += p[i, j] * ev[j - i + 2]
        np.testing.assert_allclose(got[:, c], o, atol=1e-12)
    f32 = O.mha_ref(q, k, v, 2, 4, 2.0, ek=ek, ev=ev, window=2, dtype=np.float32)
    assert 0 < np.abs(f32 - got).max() < 1e-5
    assert np.array_equal(O.seg_fill_ref(9, [0, 2, 3], [2, 1, 1], 2), np.int32([0, 0, 0, 0, 1, 1, 2, 2, -1]))


# ------------------------------------------------------------------ struct layouts
def _lib():
    from genie_tts_amd import engine
    return engine


def test_desc_structs_match_the_c_header(tmp_path):
    E = _lib()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    structs = {"gsv_conv_desc": E.ConvDesc, "gsv_mrf_desc": E.MrfDesc, "gsv_mha_desc": E.MhaDesc,
               "gsv_vits_rows_desc": E.VitsRowsDesc}
    lines = []
    for cname, S in structs.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        lines += [f'    printf("%zu\\n", offsetof({cname}, {n}));' for n, _ in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "genie_engine.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = iter(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    for cname, S in structs.items():
        assert ctypes.sizeof(S) == next(vals), cname
        for n, _ in S._fields_:
            assert getattr(S, n).offset == next(vals), (cname, n)


# ------------------------------------------------------------------ gsv_debug_conv, host side
P = 1 << 20     # an aligned stand-in pointer: the dry path and every rejection make no HIP call
BIG = 1 << 40


def _conv_fields(**f):
    """A valid f32 conv (16 -> 16, K 3, 32 columns) on stand-in pointers, fields replaced by f; with
    wh given, the f16 path's other pointers too."""
    base = dict(Cin=16, Cout=16, K=3, Tin=32, n_t=32, o_len=32, pad=1, x=P, x_cs=32, w=P, out=P, o_cs=32, r_cs=32,
                n_x=BIG, n_w=BIG, n_out=BIG, n_res=BIG, n_acc=BIG, n_out2=BIG, n_seg=BIG)
    if "wh" in f:
        base.update(w=0, wscale=P, ovf=P)
    base.update(f)
    geo = {"Tin": "x_cs", "o_len": "o_cs"}
    for k, s in geo.items():                       # keep the row strides at the row lengths unless given
        if k in f and s not in f:
            base[s] = base[k]
    if "o_len" in f and "r_cs" not in f:
        base["r_cs"] = base["o_len"]
    return base


def _form(**f):
    return _lib().debug_conv(stream=None, dry=1, **_conv_fields(**f))


def _rejected(dry=0, **f):
    E = _lib()
    form = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    rc = E.lib().gsv_debug_conv(ctypes.byref(E.conv_desc(dry=dry, **_conv_fields(**f))), None, form)
    assert rc == -1 and list(form) == [-1] * 4, (rc, list(form))     # GSV_E_ARG, before any HIP call
    msg = E.lib().gsv_last_error().decode()
    assert msg.startswith("debug conv: "), msg
    return msg


def test_debug_conv_rejects_bad_arguments_without_touching_the_gpu():
    r = _rejected
    for K in (0, 6, 8, 9, 10, 12):
        assert "K outside the f32" in r(K=K)
    for K in (0, 5, 6, 8, 12):
        assert "K outside the f16" in r(K=K, wh=P)
    for dil in (0, 6, -1):
        assert "dil outside" in r(dil=dil) and "dil outside" in r(dil=dil, wh=P)
    assert "null x" in r(x=0) and "null w" in r(w=0) and "null out" in r(out=0)
    for mode in ("resid", "sub", "acc_first", "acc_add", "acc_mean", "resid_vec", "split_resid"):
        assert "reads res" in r(mode=mode, acc=P, vec=P, out2=P, res2=P, split=4)
    for mode in ("vec", "resid_vec"):
        assert "reads vec" in r(mode=mode, res=P)
    for mode in ("acc_first", "acc_add", "acc_mean"):
        assert "acc" in r(mode=mode, res=P)
    assert "out2 and res2" in r(mode="split_resid", res=P, res2=P, split=4)
    assert "out2 and res2" in r(mode="split_resid", res=P, out2=P, split=4)
    assert "split outside" in r(mode="split_resid", res=P, out2=P, res2=P, split=17)
    assert "split outside" in r(mode="split_resid", res=P, out2=P, res2=P, split=-1)
    assert "div == 0" in r(mode="acc_mean", res=P, acc=P, div=0.0)
    assert "unknown mode" in r(mode=11) and "unknown mode" in r(mode=-1)
    # ACC_FIRST / ACC_ADD write acc alone: out may be null
    assert _form(mode="acc_first", res=P, acc=P, out=0)["path"] == "f32"
    # seg where nothing reads it, or shorter than the columns it is indexed at
    assert "seg with deferred" in r(seg=P, deferred=1, part=P, part_cap=BIG)
    assert "seg shorter" in r(seg=P, n_seg=31)
    assert "deferred needs" in r(deferred=1, part=P, part_cap=BIG, o_len=31)
    assert "deferred needs part" in r(deferred=1)
    # extents against the stated element counts
    assert "x smaller" in r(n_x=16 * 32 - 1)
    assert "x smaller" in r(x_cs=1, x_ts=16, n_x=16 * 32 - 1)                       # time-major
    assert "out smaller" in r(n_out=16 * 32 - 1)
    assert "out smaller" in r(o_cs=1, o_ts=16, n_out=16 * 32 - 1)
    assert "res smaller" in r(mode="resid", res=P, n_res=16 * 32 - 1)
    assert "acc smaller" in r(mode="acc_add", res=P, acc=P, n_acc=16 * 32 - 1)
    assert "out2 / res2 smaller" in r(mode="split_resid", res=P, out2=P, res2=P, split=5, n_out2=11 * 32 - 1)
    assert "out smaller" in r(mode="split_resid", res=P, out2=P, res2=P, split=5, n_out=5 * 32 - 1)
    assert _form(mode="split_resid", res=P, out2=P, res2=P, split=5, n_out=5 * 32, n_out2=11 * 32, n_res=5 * 32)["path"] == "f32"
    # a polyphase conv: 3 phases, n_t 12 columns each, o_toff -2, clipped at o_len 30
    poly = dict(phases=3, o_tstride=3, o_toff=-2, n_t=12, o_len=30, Tin=10, pad=2, w_phase_stride=16 * 16 * 3)
    assert _form(**poly, n_out=16 * 30, n_w=3 * 768)["path"] == "f32"
    assert "out smaller" in r(**poly, n_out=16 * 30 - 1)
    assert _form(**{**poly, "o_len": 40}, n_out=15 * 40 + 34)["path"] == "f32"      # last column 11 * 3 - 2 + 2 = 33
    assert "out smaller" in r(**{**poly, "o_len": 40}, n_out=15 * 40 + 33)
    assert "w smaller" in r(**poly, n_w=3 * 768 - 1)
    assert "w_phase_stride" in r(**{**poly, "w_phase_stride": 767})
    assert "part smaller" not in r(n_x=1)                                           # (another message)
    # the f16 path
    assert "16-B aligned" in r(wh=P + 8)
    assert "Cin % 8" in r(wh=P, Cin=20)
    assert "x_ts == 1" in r(wh=P, x_cs=1, x_ts=16)
    assert "wscale and ovf" in r(wh=P, wscale=0) and "wscale and ovf" in r(wh=P, ovf=0)
    assert "not covered by the f16 path" in r(wh=P, o_tstride=2)
    assert "not covered by the f16 path" in r(wh=P, **{**poly, "o_tstride": 2}, wh_phase_stride=768)
    assert "wh_phase_stride" in r(wh=P, **poly, wh_phase_stride=760)
    assert "wh smaller" in r(wh=P, **poly, wh_phase_stride=768, n_w=3 * 768 - 1)
    assert _form(wh=P, **poly, wh_phase_stride=768, n_w=3 * 768)["path"] == "conv_h"
    assert "in_scale" in r(in_scale=P)
    assert "tile_force" in r(wh=P, tile_force=5)
    assert "positive" in r(Cin=0) and "positive" in r(n_t=0) and "positive" in r(o_len=0)
    assert "strides" in r(x_cs=0) and "strides" in r(o_ts=0)
    # the dry path refuses the same sets
    assert "K outside" in r(dry=1, K=6) and "x smaller" in r(dry=1, n_x=3)
    E = _lib()
    form = (ctypes.c_int32 * 4)()
    assert E.lib().gsv_debug_conv(None, None, form) == -1
    assert E.lib().gsv_debug_conv(ctypes.byref(E.conv_desc(**_conv_fields())), None, None) == -1


def test_conv_form_f32_boundaries():
    f = _form
    big = dict(part=P, part_cap=BIG)
    assert f() == {"path": "f32", "nsplit": 1, "v4": True, "slabs": 0}
    # split-K below 128 blocks of 64 x 64, with a workspace, one phase and more than one Cin chunk
    assert f(Cin=192, n_t=127 * 64, Tin=127 * 64, o_len=127 * 64, **big) == {"path": "f32_splitk", "nsplit": 3, "v4": True, "slabs": 0}
    assert f(Cin=192, n_t=128 * 64, Tin=128 * 64, o_len=128 * 64, **big)["path"] == "f32"
    assert f(Cin=192, Cout=128, n_t=64 * 64, Tin=64 * 64, o_len=64 * 64, **big)["path"] == "f32"          # 64 x 2 blocks
    assert f(Cin=192, Cout=128, n_t=63 * 64, Tin=64 * 64, o_len=64 * 64, **big)["nsplit"] == 3           # 126 blocks
    assert f(Cin=192, n_t=127 * 64, Tin=127 * 64, o_len=127 * 64)["path"] == "f32"                         # no workspace
    # nsplit = min(chunks, ceil(256 / blocks)); chunks = ceil(Cin / CI), CI = 32, 32, 16, 16, 8, 8, 4 for K = 1 .. 11
    assert f(Cin=192, Cout=384, K=5, pad=2, Tin=37, n_t=37, o_len=37, **big)["nsplit"] == 24              # 6 blocks: min(24, 43)
    assert f(Cin=192, Cout=64, K=3, Tin=200, n_t=200, o_len=200, **big)["nsplit"] == 12                   # 4 blocks: min(12, 64)
    assert f(Cin=192, Cout=64, K=1, pad=0, Tin=64 * 100, n_t=64 * 100, o_len=64 * 100, **big)["nsplit"] == 3  # min(6, 3)
    assert f(Cin=20, Cout=65, K=11, pad=5, **big)["nsplit"] == 5                                           # ceil(20 / 4)
    assert f(Cin=16, K=3, **big)["path"] == "f32"                                                          # one chunk
    assert f(Cin=17, K=3, **big)["nsplit"] == 2
    # deferred reports the slabs it will leave
    assert f(Cin=192, K=3, deferred=1, **big) == {"path": "f32_splitk", "nsplit": 12, "v4": True, "slabs": 12}
    assert f(Cin=16, K=3, deferred=1, **big)["slabs"] == 0
    # part_cap cuts nsplit, down to 1
    n = 384 * 37
    geo = dict(Cin=192, Cout=384, K=5, pad=2, Tin=37, n_t=37, o_len=37, part=P)
    assert f(**geo, part_cap=24 * n)["nsplit"] == 24
    assert f(**geo, part_cap=24 * n - 1)["nsplit"] == 23
    assert f(**geo, part_cap=5 * n)["nsplit"] == 5
    assert f(**geo, part_cap=2 * n)["nsplit"] == 2
    assert f(**geo, part_cap=2 * n - 1) == {"path": "f32", "nsplit": 1, "v4": True, "slabs": 0}
    assert f(**geo, part_cap=0)["path"] == "f32"
    # phases keep a conv off split-K
    assert f(Cin=192, phases=2, o_tstride=2, n_t=16, w_phase_stride=192 * 16 * 3, **big)["path"] == "f32"
    # V4: Cin K % 4, the weight pointer, the phase stride
    assert f(Cin=3, Cout=1, K=3)["v4"] is False and f(Cin=4, K=3)["v4"] is True
    assert f(Cin=20, K=5, pad=2)["v4"] is True and f(Cin=20, K=5, pad=2, w=P + 4)["v4"] is False
    assert f(w=P + 8)["v4"] is False
    assert f(phases=2, o_tstride=2, n_t=16, w_phase_stride=16 * 16 * 3 + 2)["v4"] is False
    assert f(phases=2, o_tstride=2, n_t=16, w_phase_stride=16 * 16 * 3 + 4)["v4"] is True


def test_conv_form_f16_boundaries():
    f = lambda **k: _form(wh=P, **k)
    assert f(Cin=64) == {"path": "conv_h", "chunk": 32, "tile": 2, "slabs": 0}
    assert f(Cin=32)["chunk"] == 32 and f(Cin=96)["chunk"] == 32
    for cin in (8, 24, 48, 40):
        assert f(Cin=cin)["chunk"] == 8, cin
    # the cost model on the generator's stage shapes (V2: 256 .. 16 channels at 10, 80, 160, 320, 640 x T):
    # cost = ceil(blocks / 512) x tile area x (1 + 0.1 (KS - 1)) over (64,128,1), (32,128,2), (32,64,4), (32,256,1)
    for C, T, tile in ((256, 1000, 2), (128, 8000, 2), (64, 16000, 2), (32, 32000, 2), (16, 64000, 1),
                       (128, 80000, 1), (64, 65536, 0), (256, 16384, 0)):
        assert f(Cin=C, Cout=C, Tin=T, n_t=T, o_len=T)["tile"] == tile, (C, T)
    for tf in (1, 2, 3, 4):
        assert f(Cin=64, tile_force=tf)["tile"] == tf - 1
    # a polyphase ConvTranspose counts its phases' blocks
    assert f(Cin=32, Cout=16, K=2, pad=1, phases=10, o_tstride=10, Tin=5, n_t=6, o_len=50, wh_phase_stride=16 * 2 * 32)["path"] == "conv_h"
    # k_conv_ws: tile 0, Cin == Cout in {64, 128 (7 taps only)}, >= 2 tiles of 256 per lane, the MRF modes
    ws = dict(Cin=64, Cout=64, K=7, pad=3, Tin=4099, n_t=4099, o_len=4099, ws=8, tile_force=1)
    assert f(**ws) == {"path": "conv_ws", "chunk": 32, "tile": 0, "slabs": 0}
    assert f(**{**ws, "K": 11, "pad": 5})["path"] == "conv_ws"
    assert f(**{**ws, "Cin": 128, "Cout": 128})["path"] == "conv_ws"
    assert f(**{**ws, "Cin": 128, "Cout": 128, "K": 11, "pad": 5})["path"] == "conv_h"
    assert f(**{**ws, "Cin": 192, "Cout": 192})["path"] == "conv_h"
    assert f(**{**ws, "Cout": 128})["path"] == "conv_h"
    assert f(**{**ws, "K": 3, "pad": 1})["path"] == "conv_h"
    assert f(**{**ws, "ws": 0})["path"] == "conv_h"
    assert f(**{**ws, "ws": 9})["path"] == "conv_h"                                  # 17 tiles < 18
    assert f(**{**ws, "n_t": 3841, "Tin": 3841, "o_len": 3841})["path"] == "conv_ws"  # 16 tiles
    assert f(**{**ws, "n_t": 3840, "Tin": 3840, "o_len": 3840})["path"] == "conv_h"   # 15 tiles
    for tf in (2, 3, 4):
        assert f(**{**ws, "tile_force": tf}) == {"path": "conv_h", "chunk": 32, "tile": tf - 1, "slabs": 0}
    assert f(**{**ws, "tile_force": 0})["path"] == "conv_h"                          # the cost model picks (1,1,4) here
    big = dict(ws, n_t=65536, Tin=65536, o_len=65536, tile_force=0)
    assert f(**big)["path"] == "conv_ws"                                             # ... and (2,2,1) here
    for mode in ("resid", "acc_first", "acc_add", "acc_mean"):
        assert f(**ws, mode=mode, res=P, acc=P)["path"] == "conv_ws", mode
    for mode in ("relu", "tanh", "sub", "vec", "resid_vec", "split_resid"):
        assert f(**ws, mode=mode, res=P, vec=P, out2=P, res2=P, split=8)["path"] == "conv_h", mode


def test_convh_cfg_environment_override_still_works():
    code = ("from tests.test_vits_kernels_host import _form, P\n"
            "print(_form(wh=P, Cin=64)['tile'], _form(wh=P, Cin=64, tile_force=4)['tile'])\n")
    for env, want in (({"GENIE_CONVH_CFG": "3"}, "3 3"), ({"GENIE_CONVH_CFG": "0"}, "0 3"), ({"GENIE_CONVH_CFG": "9"}, "2 3"),
                      ({}, "2 3")):
        e = {k: v for k, v in os.environ.items() if k != "GENIE_CONVH_CFG"}
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**e, **env}, check=True, capture_output=True,
                             text=True).stdout.split("\n")[0]
        assert out == want, (env, out)


# ------------------------------------------------------------------ the other hooks, host side
def _rc(fn, desc):
    E = _lib()
    rc = fn(ctypes.byref(desc), None)
    return rc, E.lib().gsv_last_error().decode()


def test_debug_mrf_pair_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()

    def r(**f):
        d = E.MrfDesc()
        T, C = f.get("T", 100), f.get("C", 16)
        base = dict(T=T, C=C, K=3, dil=1, mode=E.CONV_MODES["resid"], Cout=C, n_t=T, o_len=T, o_tstride=1, o_toff=0,
                    div=1.0, r=P, w1=P, s1=P, b1=P, w2=P, s2=P, bias2=P, ovf=P, out=2 * P, acc=0, o_cs=T, o_ts=1,
                    r_cs=T, r_ts=1, n_r=BIG, n_out=BIG, n_acc=BIG, n_seg=BIG)
        base.update(f)
        for k, v in base.items():
            setattr(d, k, v)
        rc, msg = _rc(E.lib().gsv_debug_mrf_pair, d)
        assert rc == -1 and msg.startswith("debug mrf_pair: "), (rc, msg)
        return msg

    for k in ("w1", "w2", "s1", "s2", "b1", "ovf"):
        assert "not covered: weights" in r(**{k: 0})
    assert "not covered: dilation" in r(dil=0) and "not covered: dilation" in r(dil=6)
    for f in (dict(o_tstride=2), dict(o_toff=1), dict(o_ts=2), dict(o_cs=99), dict(Cout=15), dict(n_t=99), dict(o_len=99)):
        assert "not covered: the output" in r(**f), f
    assert "not covered: conv2's bias" in r(bias2=0) and "not covered: conv2's bias" in r(r_cs=99)
    assert "not covered: conv2's bias" in r(r_ts=2)
    for mode in ("store", "relu", "tanh", "vec", "sub", "resid_vec", "split_resid"):
        assert "not covered: modes" in r(mode=E.CONV_MODES[mode]), mode
    for K, C in ((5, 16), (1, 32), (3, 24), (7, 64), (11, 8)):
        assert "not covered: K in" in r(K=K, C=C)
    assert "null r" in r(r=0) and "null out" in r(out=0)
    for mode in ("acc_first", "acc_add", "acc_mean"):
        assert "acc" in r(mode=E.CONV_MODES[mode])
    assert "div == 0" in r(mode=E.CONV_MODES["acc_mean"], acc=3 * P, div=0.0)
    assert "16-B aligned" in r(w1=P + 8) and "16-B aligned" in r(w2=P + 2)
    assert "alias" in r(out=P) and "alias" in r(mode=E.CONV_MODES["acc_first"], acc=P)
    assert "r smaller" in r(n_r=1599) and "out smaller" in r(n_out=1599)
    assert "acc smaller" in r(mode=E.CONV_MODES["acc_add"], acc=3 * P, n_acc=1599)
    assert "seg shorter" in r(seg=P, n_seg=99)
    assert "positive" in r(T=0)
    assert E.lib().gsv_debug_mrf_pair(None, None) == -1


def test_debug_mha_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()

    def r(host=None, **f):
        d = E.MhaDesc()
        base = dict(nq=4, nk=4, heads=2, dk=8, scale=2.0, q=P, k=P, v=P, out=P, q_ts=16, q_cs=1, k_ts=16, k_cs=1,
                    v_ts=16, v_cs=1, o_ts=16, o_cs=1, n_q=BIG, n_k=BIG, n_v=BIG, n_out=BIG)
        base.update(f)
        if host is not None:
            host = np.ascontiguousarray(host, np.int32)
            base.update(row_seg=P, row_seg_host=host.ctypes.data)
        for k, v in base.items():
            setattr(d, k, v)
        rc, msg = _rc(E.lib().gsv_debug_mha, d)
        assert rc == -1 and msg.startswith("debug mha: "), (rc, msg)
        return msg

    assert "dk > 128" in r(dk=129)
    assert "key count" in r(nk=2049) and "key count" in r(nk=0)
    assert "window > 8" in r(ek=P, window=9) and "window > 8" in r(ev=P, window=9)
    assert "nq == nk" in r(ek=P, window=4, nk=5) and "nq == nk" in r(ev=P, window=4, nq=3)
    assert "key count" in r(host=[[0, 4], [0, 0], [0, 4], [0, 4]])
    assert "key count" in r(host=[[0, 4], [0, 2049], [0, 4], [0, 4]], n_k=1 << 30)
    assert "leaves the key buffer" in r(host=[[0, 4], [-1, 4], [0, 4], [0, 4]])
    assert "leaves the key buffer" in r(host=[[0, 4], [0, 4], [2, 4], [0, 4]], n_k=5 * 16 + 15)      # rows 0 .. 5
    assert "leaves the key buffer" in r(host=[[0, 4], [0, 4], [2, 4], [0, 4]], n_v=5 * 16 + 15)
    assert "own key range" in r(host=[[0, 2], [0, 2], [0, 2], [2, 2]], ek=P, window=4)
    assert "host copy" in r(row_seg=P)
    assert "q smaller" in r(n_q=3 * 16 + 15) and "out smaller" in r(n_out=3 * 16 + 15)
    assert "leaves the key buffer" in r(n_k=3 * 16 + 15) and "leaves the key buffer" in r(n_v=3 * 16 + 15)
    assert "q smaller" in r(q_ts=1, q_cs=4, n_q=63)                                                    # channel-major
    assert "null" in r(q=0) and "null" in r(out=0)
    assert "scale" in r(scale=0.0)
    assert "positive" in r(nq=0) and "positive" in r(heads=0)
    assert E.lib().gsv_debug_mha(None, None) == -1


def test_debug_vits_rows_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()

    def r(op, **f):
        d = E.VitsRowsDesc()
        base = dict(op=E.VITS_ROW_OPS[op] if isinstance(op, str) else op, C=192, T=5, nsplit=2, nseg=2, f=1, n=10, div=3.0,
                    x=P, y=P, z=P, out=P, g=P, b=P, bias=P, vec=P, off=P, len=P)
        base.update(f)
        for k, v in base.items():
            setattr(d, k, v)
        return _rc(E.lib().gsv_debug_vits_rows, d)

    def no(op, what, **f):
        rc, msg = r(op, **f)
        assert rc == -1 and msg.startswith("debug vits rows: ") and what in msg, (op, f, rc, msg)

    no("ln_channels", "C <= 256", C=257)
    no("ln_channels", "C <= 256", C=272)                  # a multiple of 16 past the narrow form
    no("ln_channels", "seg needs", C=100, seg=P)
    no("ln_channels", "g and b", g=0)
    no("ln_channels", "null x", x=0)
    no("ln_channels", "positive", C=0)
    no("ln_channels_slabs", "C % 16", C=100)
    no("ln_channels_slabs", "C <= 256", C=272)
    no("ln_channels_slabs", "nsplit >= 2", nsplit=1)
    no("ln_channels_slabs", "nsplit >= 2", y=0)
    no("wn_gate_slabs", "nsplit >= 1", nsplit=0)
    no("wn_gate_slabs", "reads vec", vec=0)
    no("wn_gate", "null x", x=0)
    no("mean3", "mean3 needs", z=0)
    no("mean3", "mean3 needs", n=-1)
    no("mean3", "div == 0", div=0.0)
    no("seg_fill", "nseg >= 1", nseg=0)
    no("seg_fill", "nseg >= 1", f=0)
    no("seg_fill", "off, len", off=0)
    no(6, "op:")
    no("mean3", "null out", out=0)
    # nothing to do: success without a launch
    for op in ("ln_channels", "ln_channels_slabs", "wn_gate", "wn_gate_slabs"):
        assert r(op, T=0)[0] == 0, op
    for op in ("mean3", "seg_fill"):
        assert r(op, n=0)[0] == 0, op
    assert E.lib().gsv_debug_vits_rows(None, None) == -1
