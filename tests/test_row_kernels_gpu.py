"""GPU: the row kernels around the GEMM (csrc/t2s.hip, csrc/hubert.hip), one launch at a time through
gsv_debug_rows, against fp64.  Tolerances come from fp32 CPU references (tests/NUMERICS.md)."""
import numpy as np
import pytest
import torch

from tests import gemm_oracle as O

pytestmark = pytest.mark.gpu

MARGIN = 4.0
CONST = 0.75            # sums of up to 1024 copies are exact in fp32: a constant row must give b exactly


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_rows_input, _ln_rho = O.ln_rows, O.ln_rho


def _check_ln(out, v, g, b, eps, what):
    t = torch.nn.functional.layer_norm(torch.from_numpy(v), (v.shape[1],), torch.from_numpy(g), torch.from_numpy(b),
                                       eps).numpy()
    bar = MARGIN * _ln_rho(t, v, g, b, eps)
    r = _ln_rho(out, v, g, b, eps)
    print(f"LN {what} rows={v.shape[0]} D={v.shape[1]} eps={eps:g}: rho {r:.3g} bar {bar:.3g}")
    assert np.all(np.isfinite(out)) and r <= bar, (what, r, bar)
    if v.shape[0] == 3:
        assert np.array_equal(out[1], b), "a constant row is b exactly"


def _gb(D, rng):
    return (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)


LN_CASES = [("layernorm_rows", 512, 1e-5)] + [("layernorm_rows_d", D, eps) for D in (512, 768, 1024, 300)
                                                for eps in (1e-5, 1e-12)]


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("op,D,eps", LN_CASES)
def test_layernorm(op, D, eps, rows):
    from genie_tts_amd.engine import debug_rows
    rng = np.random.default_rng([D, rows])
    x, (g, b) = _rows_input(rows, D, rng), _gb(D, rng)
    out = torch.full((rows + 1, D), 7.0, device="cuda")
    debug_rows(op, rows, D, _dev(x), out, g=_dev(g), b=_dev(b), eps=eps)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[rows:] == 7.0)
    _check_ln(o[:rows], x, g, b, eps, op)


SLAB_CASES = [("layernorm_rows_slabs", 512, 1e-5)] + [("layernorm_rows_d_slabs", D, eps)
                                                       for D, eps in ((512, 1e-5), (768, 1e-12), (1024, 1e-5),
                                                                      (300, 1e-12))]


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("nslab", [1, 4, 8])
@pytest.mark.parametrize("op,D,eps", SLAB_CASES)
def test_layernorm_slabs(op, D, eps, nslab, rows):
    """LayerNorm of res + (bias + the slabs summed in order), the sum restated in fp32."""
    from genie_tts_amd.engine import debug_rows
    rng = np.random.default_rng([D, rows, nslab])
    res, (g, b) = _rows_input(rows, D, rng), _gb(D, rng)
    slabs = rng.standard_normal((nslab, rows + 2, D)).astype(np.float32)      # 2 rows of slack per slab
    bias = rng.standard_normal(D).astype(np.float32)
    if rows == 3:                                # the constant row: slab 0 cancels the shared bias, the rest add 0
        slabs[:, 1] = 0
        slabs[0, 1] = -bias
    p = np.zeros((rows, D), np.float32)
    for z in range(nslab):
        p = p + slabs[z, :rows]
    v = res + (bias[None, :] + p)
    assert rows == 1 or np.all(v[1] == CONST)
    assert v.dtype == np.float32
    out = torch.full((rows + 1, D), 7.0, device="cuda")
    f = dict(g=_dev(g), b=_dev(b), eps=eps, nslab=nslab, slab_stride=(rows + 2) * D, bias=_dev(bias), res=_dev(res))
    planes = op == "layernorm_rows_slabs"
    if planes:
        hi, lo = (torch.full((rows + 1, D), 7.0, dtype=torch.float16, device="cuda") for _ in range(2))
        f.update(out_hi=hi, out_lo=lo)
    debug_rows(op, rows, D, _dev(slabs), out, **f)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[rows:] == 7.0)
    _check_ln(o[:rows], v, g, b, eps, f"{op} nslab={nslab}")
    if planes:                                   # the planes are the split of the stored f32 values
        ehi, elo = O.split_a(o[:rows])
        assert np.array_equal(hi.cpu().numpy()[:rows], ehi) and np.array_equal(lo.cpu().numpy()[:rows], elo)
        assert np.all(hi.cpu().numpy()[rows:] == 7.0) and np.all(lo.cpu().numpy()[rows:] == 7.0)
        out2 = torch.full((rows + 1, D), 7.0, device="cuda")                  # without planes: the same f32
        f.pop("out_hi"), f.pop("out_lo")
        debug_rows(op, rows, D, _dev(slabs), out2, **f)
        torch.cuda.synchronize()
        assert torch.equal(out, out2)


@pytest.mark.parametrize("op", ["layernorm_rows", "layernorm_rows_slabs", "layernorm_rows_d", "layernorm_rows_d_slabs",
                                "sumsq_rows", "argmin_dist_rows"])
def test_zero_rows_is_success_without_a_launch(op):
    from genie_tts_amd.engine import debug_rows
    x = torch.zeros(1024, device="cuda")
    out = torch.full((1024,), 7.0, device="cuda")
    f = dict(g=x, b=x, eps=1e-5) if op.startswith("layernorm") else {}
    if op.endswith("slabs"):
        f.update(nslab=2, slab_stride=512, bias=x, res=x)
    debug_rows(op, 0, 512, x, out, ld=512, **f)
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)


@pytest.mark.parametrize("cols", [1, 255, 768, 1000])
def test_sumsq_rows(cols):
    """The bar: MARGIN times the relative error of an fp32 sum of the fp32 squares in order of c,
    the worst of 64 rows."""
    from genie_tts_amd.engine import debug_rows
    rows, ld = 64, cols + 3
    rng = np.random.default_rng(cols)
    x = np.full((rows, ld), np.nan, np.float32)
    x[:, :cols] = rng.standard_normal((rows, cols)).astype(np.float32)
    v = x[:, :cols]
    ref = (v.astype(np.float64) ** 2).sum(1)
    seq = np.zeros(rows, np.float32)
    for c in range(cols):
        seq = seq + v[:, c] * v[:, c]
    bar = MARGIN * float(np.max(np.abs(seq - ref) / ref))
    out = torch.full((rows + 1,), 7.0, device="cuda")
    debug_rows("sumsq_rows", rows, cols, _dev(x), out, ld=ld)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    r = float(np.max(np.abs(o[:rows] - ref) / ref))
    print(f"SUMSQ cols={cols}: rel err {r:.3g} bar {bar:.3g}")
    assert o[rows] == 7.0 and r <= bar


@pytest.mark.parametrize("cols", [1, 256, 257, 1024])
def test_argmin_dist_rows_first_index_ties(cols):
    """Exact ties across lanes (i, i + 1), waves (i, i + 64) and strides of one thread (i, i + 256)
    return the lowest index; a row of equal values returns 0."""
    from genie_tts_amd.engine import debug_rows
    ties = [(700, 300, 301), (129, 65), (517, 261), (1023, 3), (), (456, 200, 10), (256, 0), (256, 255), (255, 254)]
    rng = np.random.default_rng(cols)
    dist = (1.0 + rng.random((len(ties) + 1, cols))).astype(np.float32)
    for r, t in enumerate(ties):
        for i in t:
            if i < cols:
                dist[r, i] = 0.5
    dist[4] = 1.25                                       # all equal
    exp = np.argmin(dist, axis=1)                        # numpy: the first of equal minima
    assert exp[4] == 0 and (cols < 1024 or list(exp[:4]) == [300, 65, 261, 3])
    out = torch.full((len(ties) + 2,), -7, dtype=torch.int64, device="cuda")
    debug_rows("argmin_dist_rows", len(ties) + 1, cols, _dev(dist), out)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(o[:-1], exp) and o[-1] == -7
