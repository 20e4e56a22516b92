"""CPU: the T2S kernel oracle (tests/t2s_oracle.py) against plain restatements, the sharpness of its
bars against wrong attentions, the layouts of the debug-hook structs, every argument rejection of
gsv_debug_attn / _attn_out / _gemv / _ffn / _embed (GSV_E_ARG with no HIP call) and attn_form's
boundaries.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import t2s_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the lengths the GPU tests run each input family at (tests/test_t2s_kernels_gpu.py imports these)
LENS_ROWS = (1, 2, 8, 9, 57, 64, 65, 255, 256, 257, 512, 513, 1030)
LENS_FLASH = (1, 63, 64, 65, 128, 129, 193)
LENS_MF32 = LENS_FLASH + (192, 257)
LENS_OUT = (1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1024, 1025)
LENS_PEAKED = (129, 513)
LENS_TILES = (70, 160, 161)          # the causal-tile and packed-prefill cases' longest lengths
UNIT_LENS = sorted(set(LENS_ROWS + LENS_MF32 + LENS_OUT + LENS_TILES))


# ------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("T", [1, 2, 65, 200])
def test_fp64_attention_is_the_dense_softmax_form(T):
    q, K, V = O.UNIT.data(3, 1, 256)
    got = O.attn_rows(q, K[0], V[0], [T] * 3)
    qh = torch.from_numpy(q.astype(np.float64)).reshape(3, 16, 32).permute(1, 0, 2) * O.SCALE
    kh, vh = (torch.from_numpy(a[0, :, :T].astype(np.float64)) for a in (K, V))
    ref = (torch.softmax(qh @ (kh * O.SCALE).transpose(1, 2), -1) @ vh).permute(1, 0, 2).reshape(3, 512).numpy()
    assert np.abs(got - ref).max() < 1e-14


@pytest.mark.parametrize("fam", [O.UNIT, O.PEAKED], ids=["unit", "peaked"])
@pytest.mark.parametrize("mode", ["f32", "fast_exp"])
def test_fp32_modes_are_fp32_level(fam, mode):
    for T in (1, 65, 513):
        q, K, V = fam.data(4, 1, 520)
        ref = O.attn_rows(q, K[0], V[0], [T] * 4)
        got = O.attn_rows(q, K[0], V[0], [T] * 4, mode=mode)
        assert got.dtype == np.float32
        e = np.abs(got - ref).max()
        assert e < 1e-5, (T, e)
        if T == 1:
            assert e == 0                                          # one key: P = 1, the output is V's row


def test_one_key_bar_is_not_zero():
    assert O.UNIT.bar(1, "f32") == O.UNIT.bar(O.BAR_MIN_KEYS + O.BAR_ROWS, "f32") > 1e-7


def test_fixed_point_round_trip():
    v = np.float32([0.0, 1.0, -1.5, 3.0e-10, 123.456])
    assert np.array_equal(O.fx(v), np.rint(v.astype(np.float64) * 2.0 ** 32).astype(np.int64))
    assert np.abs(O.from_fx(O.fx(v)) - v).max() <= 2.0 ** -33 + 2.0 ** -24 * 124


# ------------------------------------------------------------------ sharpness
def _wrongs(T, qk):
    """The wrong attentions that apply to a family at longest length T (NUMERICS.md): a dropped or
    extra key moves a peaked softmax by as little as 1e-16, so the peaked family answers for the
    skipped rescale and the q-only scale alone; a skipped rescale at the second chunk is no defect
    until the running maximum can rise there (at least two full chunks)."""
    w = []
    if qk == 1.0:
        w += ["drop_last", "one_more", "drop_64", "no_new_row"]
    w += ["q_scale_only"]
    if T >= 128:
        w += ["skip_rescale"]
    return w


def sharp(fam, T, margin=O.MARGIN):
    """bar <= half of every row's error under every wrong attention that applies."""
    out = []
    for mode in ("f32", "fast_exp"):
        bar = fam.bar(T, mode, margin)
        for w in _wrongs(T, fam.qk):
            worst = float(fam.err(T, None, w).min())
            out.append((mode, w, bar, worst))
    return out


@pytest.mark.parametrize("T", UNIT_LENS)
def test_attention_bar_is_sharp_unit(T):
    for mode, w, bar, least in sharp(O.UNIT, T, max(O.KERNEL_MARGIN.values())):
        print(f"SHARP unit T={T} {mode} {w}: bar {bar:.3g} least error {least:.3g}")
        assert bar <= 0.5 * least, (mode, w, bar, least)


@pytest.mark.parametrize("T", LENS_PEAKED)
def test_attention_bar_is_sharp_peaked(T):
    for mode, w, bar, least in sharp(O.PEAKED, T, max(O.KERNEL_MARGIN.values())):
        print(f"SHARP peaked T={T} {mode} {w}: bar {bar:.3g} least error {least:.3g}")
        assert bar <= 0.5 * least, (mode, w, bar, least)


def test_sharpness_fails_for_a_bar_raised_too_far():
    T = 1030
    least = min(float(O.UNIT.err(T, None, w).min()) for w in _wrongs(T, 1.0))
    m = 0.6 * least / float(O.UNIT.err(T, "f32").max())
    assert any(bar > 0.5 * l for _, _, bar, l in sharp(O.UNIT, T, m))
    assert O.MARGIN <= max(O.KERNEL_MARGIN.values()) <= 16


# ------------------------------------------------------------------ struct layouts
def _lib():
    from genie_tts_amd import engine
    return engine


def test_desc_structs_match_the_c_header(tmp_path):
    E = _lib()
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    structs = {"gsv_attn_desc": E.AttnDesc, "gsv_attn_out_desc": E.AttnOutDesc, "gsv_gemv_desc": E.GemvDesc,
               "gsv_ffn_desc": E.FfnDesc, "gsv_embed_desc": E.EmbedDesc}
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
    assert all("gsv_debug_" + n in E.EXPORTED for n in ("attn", "attn_out", "gemv", "ffn", "embed"))


# ------------------------------------------------------------------ rejections: no HIP call
P = 1 << 20     # an aligned stand-in pointer: the dry path and every rejection make no HIP call
TM = 320


def _attn(form="rows", **f):
    """A valid description of 4 rows on stand-in pointers (host copies real), fields replaced by f."""
    rows = f.get("rows", 4)
    base = dict(rows=rows, tmax=TM, q=P, k=P, v=P, out=P, row_len=P, row_len_host=np.full(max(rows, 1), 5, np.int32),
                seq_stride=16 * TM * 32)
    if form in ("rowlane", "mf32"):
        base.update(tiles=P, tiles_host=np.int32([[0, 0, rows]]), ntiles=1)
    if form == "dec_slabs":
        base.update(nslab=2, slabs=P, slab_stride=rows * 1536, b_in=P, row_skip=P, q=0)
    base.update(f)
    return _lib().attn_desc(form, **base)


def _attn_rejected(form="rows", dry=0, **f):
    E = _lib()
    ran = ctypes.c_int32(7)
    rc = E.lib().gsv_debug_attn(ctypes.byref(_attn(form, dry=dry, **f)), None, ctypes.byref(ran))
    msg = E.lib().gsv_last_error().decode()
    assert rc == -1 and ran.value == -1 and msg.startswith("debug attn: "), (rc, ran.value, msg)     # GSV_E_ARG
    return msg


def _attn_form(form="auto", **f):
    E = _lib()
    ran = ctypes.c_int32(7)
    rc = E.lib().gsv_debug_attn(ctypes.byref(_attn(form, dry=1, **f)), None, ctypes.byref(ran))
    assert rc == 0, E.lib().gsv_last_error().decode()
    return E.ATTN_FORMS[ran.value]


def auto_form():
    """What attn_rows runs for one sequence's rows: k_attn_flash unless GENIE_ATTN_FLASH reads as 0 (atoi)."""
    e = os.environ.get("GENIE_ATTN_FLASH")
    m = re.match(r"\s*[+-]?\d+", e) if e is not None else None
    return "rows" if e is not None and (int(m.group()) if m else 0) == 0 else "flash"


ALL = ("auto", "rows", "flash", "rowlane", "mf32", "dec_slabs")
lens = lambda *v: np.int32(v)


def test_debug_attn_rejects_bad_arguments_without_touching_the_gpu():
    r = _attn_rejected
    for form in ALL:
        assert "positive" in r(form, rows=0) and "positive" in r(form, rows=-1) and "positive" in r(form, tmax=0)
        for k in ("k", "v", "out"):
            assert "null k, v or out" in r(form, **{k: 0})
        assert "row_len" in r(form, row_len=0) and "host copy" in r(form, row_len_host=None)
        assert "outside [1, tmax]" in r(form, row_len_host=lens(5, 5, TM + 1, 5))
        assert "16-B aligned" in r(form, k=P + 4) and "16-B aligned" in r(form, v=P + 8)
        assert "seq_stride must be" in r(form, seq_stride=16 * TM * 32 + 2)
        # the dry path refuses the same sets
        assert "positive" in r(form, dry=1, rows=0)
    for form in ALL[:-1]:
        assert "null q" in r(form, q=0) and "16-B aligned" in r(form, q=P + 4)
        assert "ldq" in r(form, ldq=514) and "ldq" in r(form, ldq=508)
        assert "outside [1, tmax]" in r(form, row_len_host=lens(5, 0, 5, 5))
        assert "outside [1, tmax]" in r(form, row_len_host=lens(-3, 5, 5, 5))
    # len_add counts: 5 + (-5) = 0 keys, tmax - 1 + 2 keys
    assert "outside [1, tmax]" in r("rows", len_add=-5) and "outside [1, tmax]" in r("rows", len_add=TM - 4)
    assert _attn_form("rows", len_add=TM - 5) == "rows" and _attn_form("rows", len_add=0) == "rows"
    for form in ("auto", "flash", "rowlane", "mf32", "dec_slabs"):
        assert "len_add" in r(form, len_add=1)
    # the LDS score array of k_attn_rows / k_attn_dec_slabs
    big = dict(tmax=5000, seq_stride=16 * 5000 * 32)
    assert "4096" in r("rows", row_len_host=lens(5, 4097, 5, 5), **big)
    assert "4096" in r("rows", row_len_host=lens(5, 4090, 5, 5), len_add=7, **big)
    assert "4096" in r("dec_slabs", row_len_host=lens(5, 4096, 5, 5), **big)
    assert _attn_form("rows", row_len_host=lens(5, 4096, 5, 5), **big) == "rows"
    assert _attn_form("dec_slabs", row_len_host=lens(5, 4095, 5, 5), **big) == "dec_slabs"
    assert _attn_form("flash", row_len_host=lens(5, 5000, 5, 5), **big) == "flash"
    # float4 stores of rowlane / mf32
    for form in ("rowlane", "mf32"):
        assert "float4" in r(form, ldo=514) and "float4" in r(form, out=P + 8)
        assert "tile table" in r(form, tiles=0)
        assert "host copy" in r(form, tiles_host=None) and "ntiles" in r(form, ntiles=0)
    assert _attn_form("flash", ldo=514, out=P + 8) == "flash" and _attn_form("rows", ldo=513, out=P + 4) == "rows"
    assert "ldo below" in r("rows", ldo=511)
    # the grid's y extent of the kernel launched: a block per row, or per 16 rows of k_attn_flash
    many = lambda n: dict(rows=n, row_len_host=np.full(n, 5, np.int32))
    assert "grid's y extent" in r("rows", **many(65536)) and _attn_form("rows", **many(65535)) == "rows"
    assert "grid's y extent" in r("auto", row_skip=P, **many(65536))
    assert _attn_form("flash", **many(16 * 65535)) == "flash" and "grid's y extent" in r("flash", **many(16 * 65535 + 1))
    if auto_form() == "flash":
        assert _attn_form("auto", **many(16 * 65535)) == "flash" and "grid's y extent" in r("auto", **many(16 * 65535 + 1))
    else:
        assert "grid's y extent" in r("auto", **many(65536))
    # tiles
    tl = lambda *t: dict(tiles=P, tiles_host=np.int32(t), ntiles=len(t), rows=200, row_len_host=np.full(200, 9, np.int32))
    for form, cap in (("flash", 16), ("rowlane", 128), ("mf32", 128)):
        assert _attn_form(form, **tl([0, 0, cap], [0, 200 - cap, cap])) == form
        assert "a block holds" in r(form, **tl([0, 0, cap + 1])) and "a block holds" in r(form, **tl([0, 0, 1], [0, 5, 0]))
        assert "past rows" in r(form, **tl([0, 200 - cap + 1, cap])) and "past rows" in r(form, **tl([0, -1, 2]))
        assert "sequence < 0" in r(form, **tl([-1, 0, 4]))
        # a second sequence needs a stride of one cache
        assert "below one cache" in r(form, seq_stride=16 * TM * 32 - 4, **tl([0, 0, 4], [1, 4, 4]))
        assert _attn_form(form, seq_stride=0, **tl([0, 0, 4], [0, 4, 4])) == form
        assert "neither row_seq nor row_skip" in r(form, row_skip=P, **tl([0, 0, 4]))
        assert "neither row_seq nor row_skip" in r(form, row_seq=P, row_seq_host=np.zeros(200, np.int32), **tl([0, 0, 4]))
    assert "neither row_seq nor row_skip" in r("flash", row_skip=P)
    assert "neither row_seq nor row_skip" in r("flash", row_seq=P, row_seq_host=lens(0, 0, 0, 0))
    for form in ("auto", "rows"):
        assert "no tile table" in r(form, tiles=P, tiles_host=np.int32([[0, 0, 4]]), ntiles=1)
        assert "host copy" in r(form, row_seq=P) and "sequence < 0" in r(form, row_seq=P, row_seq_host=lens(0, -1, 0, 0))
        assert "below one cache" in r(form, row_seq=P, row_seq_host=lens(0, 1, 0, 0), seq_stride=16 * TM * 32 - 4)
        assert _attn_form(form, row_seq=P, row_seq_host=lens(0, 0, 0, 0), seq_stride=0) == "rows"
    # dec_slabs
    d = "dec_slabs"
    assert "nslab" in r(d, nslab=0) and "null slabs or b_in" in r(d, b_in=0) and "null slabs or b_in" in r(d, slabs=0)
    assert "kvlen" in r(d, row_len=0) and "null done" in r(d, row_skip=0)
    assert "kvlen[b] + 1" in r(d, row_len_host=lens(5, TM, 5, 5)) and "kvlen[b] + 1" in r(d, row_len_host=lens(-1, 5, 5, 5))
    assert _attn_form(d, row_len_host=lens(0, TM - 1, 5, 5)) == d
    assert "overlap" in r(d, slab_stride=4 * 1536 - 4) and _attn_form(d, nslab=1, slab_stride=0) == d
    assert "below one cache" in r(d, seq_stride=16 * TM * 32 - 4) and _attn_form(d, rows=1, seq_stride=0, slab_stride=1536) == d
    assert "no row_seq and no tiles" in r(d, tiles=P, tiles_host=np.int32([[0, 0, 1]]), ntiles=1)
    E = _lib()
    assert E.lib().gsv_debug_attn(None, None, ctypes.byref(ctypes.c_int32())) == -1
    assert E.lib().gsv_debug_attn(ctypes.byref(_attn()), None, None) == -1
    assert "form: 0 .. 5" in r(6) and "form: 0 .. 5" in r(-1)


def test_attn_form_boundaries():
    assert _attn_form("auto") == auto_form()
    assert _attn_form("auto", rows=1) == auto_form() and _attn_form("auto", rows=17) == auto_form()
    assert _attn_form("auto", row_seq=P, row_seq_host=lens(0, 0, 0, 0)) == "rows"
    assert _attn_form("auto", row_skip=P) == "rows"
    assert _attn_form("auto", row_skip=P, row_seq=P, row_seq_host=lens(0, 0, 0, 0)) == "rows"
    for form in ALL[1:]:
        assert _attn_form(form) == form


def test_attn_flash_environment_switch_still_works():
    code = ("from tests.test_t2s_kernels_host import _attn_form, P\n"
            "print(_attn_form('auto'), _attn_form('auto', row_skip=P), _attn_form('flash'))\n")
    for env, want in (({"GENIE_ATTN_FLASH": "0"}, "rows rows flash"), ({"GENIE_ATTN_FLASH": "1"}, "flash rows flash"),
                      ({}, "flash rows flash")):
        e = {k: v for k, v in os.environ.items() if k != "GENIE_ATTN_FLASH"}
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**e, **env}, check=True, capture_output=True,
                             text=True).stdout.split("\n")[0]
        assert out == want, (env, out)


def _rejecter(fn_name, Desc, prefix, base):
    E = _lib()
    keep = []

    def r(**f):
        d = Desc()
        b = dict(base)
        b.update(f)
        for k, v in b.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data
            setattr(d, k, v)
        rc = getattr(E.lib(), fn_name)(ctypes.byref(d), None)
        msg = E.lib().gsv_last_error().decode()
        assert rc == -1 and msg.startswith(prefix), (f, rc, msg)
        return msg
    return r


def test_debug_attn_out_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()
    r = _rejecter("gsv_debug_attn_out", E.AttnOutDesc, "debug attn_out: ",
                  dict(B=3, tmax=TM, scale=1.0, q=P, k=P, v=P, seq_stride=16 * TM * 32, kvlen=P,
                       kvlen_host=lens(0, 5, TM - 1), WoT=P, part=P, acc_bstride=512))
    assert "positive" in r(B=0) and "positive" in r(B=-2) and "positive" in r(tmax=0)
    for k in ("q", "k", "v", "WoT", "kvlen", "kvlen_host"):
        assert "null" in r(**{k: 0})
    for k in ("q", "k", "v", "WoT"):
        assert "16-B aligned" in r(**{k: P + 8})
    assert "kvlen[b] + 1" in r(kvlen_host=lens(0, TM, 5)) and "kvlen[b] + 1" in r(kvlen_host=lens(0, -1, 5))
    assert "exactly one" in r(part=0) and "exactly one" in r(acc_out=P)
    assert "acc_bstride" in r(part=0, acc_out=P, acc_bstride=511)
    assert "below one cache" in r(seq_stride=16 * TM * 32 - 4) and "multiple of 4" in r(seq_stride=16 * TM * 32 + 1)
    assert E.lib().gsv_debug_attn_out(None, None) == -1


def test_debug_gemv_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()
    r = _rejecter("gsv_debug_gemv", E.GemvDesc, "debug gemv: ",
                  dict(B=3, N=512, K=512, mode=0, src=P, lds=512, W=P, C=P, ldc=512))
    ln = dict(ln_g=P, ln_b=P)
    part = dict(part=P, n_part=32, part_stride=3 * 512, part_bias=P, part_res=P, src=0, **ln)
    acc = dict(acc_in=P, acc_bstride=512, part_bias=P, part_res=P, src=0, **ln)
    qkv = dict(mode=3, N=1536, kv_k=P, kv_v=P, kv_tmax=TM, kv_pos0=7, kv_seq_stride=16 * TM * 32)
    for B in (0, -1, 9, 64):
        assert "B outside" in r(B=B) and "B outside" in r(B=B, **ln)
    for K in (0, 256, 1024, 4096):
        assert "K: 512 or 2048" in r(K=K, lds=4096)
    assert "N must be" in r(N=0) and "N must be" in r(N=-4)
    assert "K = 512" in r(K=2048, lds=2048, **ln) and "without ln_b" in r(ln_g=P)
    assert "LayerNorm prologue only" in r(part=P, n_part=32, part_stride=2048, part_bias=P, part_res=P)
    assert "LayerNorm prologue only" in r(acc_in=P, acc_bstride=512, part_bias=P, part_res=P)
    for n in (0, -16, 8, 17, 40):
        assert "multiple of 16" in r(**{**part, "n_part": n})
    assert "both part and acc_in" in r(**{**part, "acc_in": P})
    assert "part_bias and part_res" in r(**{**part, "part_bias": 0}) and "part_bias and part_res" in r(**{**acc, "part_res": 0})
    assert "overlap" in r(**{**part, "part_stride": 3 * 512 - 1}) and "acc_bstride" in r(**{**acc, "acc_bstride": 500})
    assert "null src" in r(src=0) and "null src" in r(src=0, **ln)
    assert "lds % 4" in r(lds=514) and "lds % 4" in r(src=P + 4) and "lds below" in r(lds=508)
    assert "W must be" in r(W=0) and "W must be" in r(W=P + 8)
    assert "null C" in r(C=0) and "ldc below" in r(ldc=511)
    assert "EPI_RESID" in r(mode=2) and "EPI_RESID" in r(mode=2, res=P, ldr=511)
    for m in (-1, 4, 5, 6, 8):
        assert "mode:" in r(mode=m)
    assert "N == 1536" in r(**{**qkv, "N": 512}) and "N == 1536" in r(**{**qkv, "ldc": 511})
    assert "caches" in r(**{**qkv, "kv_k": 0}) and "caches" in r(**{**qkv, "kv_v": 0}) and "caches" in r(**{**qkv, "kv_tmax": 0})
    assert "past tmax" in r(**{**qkv, "kv_pos0": TM}) and "past tmax" in r(**{**qkv, "kv_pos0": -1})
    assert "host copy" in r(kv_row_pos=P, **qkv)
    assert "past tmax" in r(kv_row_pos=P, kv_row_pos_host=lens(0, TM, 3), **qkv)
    assert "below one cache" in r(**{**qkv, "kv_seq_stride": 16 * TM * 32 - 1})
    assert E.lib().gsv_debug_gemv(None, None) == -1


def test_debug_ffn_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()
    r = _rejecter("gsv_debug_ffn", E.FfnDesc, "debug ffn: ",
                  dict(B=3, nslices=32, h=P, bo=P, attn_part=P, ln_g=P, ln_b=P, h1=P, W1=P, b1=P, W2T=P, part=P,
                       acc_bstride=512))
    for n in (0, 16, 33, 48, 128):
        assert "nslices" in r(nslices=n)
    for B in (0, -1, 9):
        assert "B outside" in r(B=B)
    for k in ("h", "bo", "ln_g", "ln_b", "h1", "W1", "b1", "W2T"):
        assert "null tensor" in r(**{k: 0})
    assert "attn_part and acc_attn" in r(attn_part=0) and "attn_part and acc_attn" in r(acc_attn=P)
    assert "part and acc_out" in r(part=0) and "part and acc_out" in r(acc_out=P)
    assert "16-B aligned" in r(W1=P + 8) and "16-B aligned" in r(W2T=P + 2)
    assert "acc_bstride" in r(part=0, acc_out=P, acc_bstride=511) and "acc_bstride" in r(attn_part=0, acc_attn=P, acc_bstride=0)
    assert E.lib().gsv_debug_ffn(None, None) == -1


def test_debug_embed_rejects_bad_arguments_without_touching_the_gpu():
    E = _lib()
    y = np.zeros((2, 8), np.int64)
    y[0, 2], y[1, 4] = 1024, 3
    dec = dict(op=0, n=2, n_tok=1025, n_pe=64, tok=P, tok_host=y, ldy=8, ny=P, ny_host=lens(3, 5), emb=P, alpha=P, pe=P, out=P)
    r = _rejecter("gsv_debug_embed", E.EmbedDesc, "debug embed: ", dec)
    assert "op:" in r(op=3) and "op:" in r(op=-1)
    assert "n outside" in r(n=0) and "null out" in r(out=0)
    for k in ("tok", "tok_host", "emb", "alpha", "pe"):
        assert "null tok" in r(**{k: 0}) and "null tok" in r(op=1, **{k: 0})
    assert "ny" in r(ny=0) and "ny" in r(ny_host=0) and "ny" in r(ldy=0)
    assert "ny[b] outside" in r(ny_host=lens(0, 5)) and "ny[b] outside" in r(ny_host=lens(3, 9))
    assert "pe row" in r(n_pe=5)
    assert "outside the table" in r(n_tok=1024)
    bad = y.copy()
    bad[1, 4] = -1
    assert "outside the table" in r(tok_host=bad)
    toks = np.int64([0, 5, 1024])
    aud = dict(op=1, n=3, tok_host=toks, n_pe=4)
    assert "pe row" in r(**{**aud, "n_pe": 3}) and "outside the table" in r(**{**aud, "n_tok": 1024})
    assert "outside the table" in r(**{**aud, "tok_host": np.int64([0, -1, 3])})
    assert "null ssl" in r(op=2, n=7)
    assert E.lib().gsv_debug_embed(None, None) == -1
