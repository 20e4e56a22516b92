"""GPU: the T2S decoder's own kernels launched alone through the engine-free hooks (gsv_debug_attn,
gsv_debug_attn_out, gsv_debug_gemv, gsv_debug_ffn, gsv_debug_embed) and held to bars that come from
fp64 / fp32 CPU references (tests/t2s_oracle.py, tests/NUMERICS.md).  Every output, accumulator and
cache sits between sentinel-filled margins that must come back untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_oracle as G
from tests import t2s_oracle as O
from tests.test_t2s_kernels_host import LENS_FLASH, LENS_MF32, LENS_OUT, LENS_PEAKED, LENS_ROWS, auto_form

pytestmark = pytest.mark.gpu

SENT = 777.25            # the sentinel of margins and of never-written elements
ISENT = 7 << 40          # ... of the int64 accumulators
MARGIN = 64              # elements on both sides (a multiple of 16 B for every type used)
TMAX, TLONG = 320, 1056
CAP = {"flash": 16, "rowlane": 128, "mf32": 128}
PREFILL = ("flash", "rowlane", "mf32")


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
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the families' arrays are read-only


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def caches(fam, rows, nseq, tmax, longest, stale=0.0):
    """(q, K, V) of a family with every cache position at or past its sequence's longest visible
    length (longest[s]; 0: a sequence no row addresses) set to `stale`."""
    q, K, V = fam.data(rows, nseq, tmax)
    K, V = K.copy(), V.copy()
    for s in range(nseq):
        K[s, :, longest[s]:], V[s, :, longest[s]:] = stale, stale
    return q, K, V


def run_attn(form, q, K, V, lens, *, seqs=None, tiles=None, skip=None, len_add=0, ldo=512):
    """One gsv_debug_attn launch of a prefill / row form.  K, V [nseq][16][tmax][32]; returns out
    [rows][ldo] (never-written elements SENT) after checking that the caches came back untouched."""
    rows, (nseq, _, tmax, _) = len(lens), K.shape
    gk, gv, out = Guard(K.size, K), Guard(V.size, V), Guard(rows * ldo)
    f = dict(rows=rows, tmax=tmax, q=dev(q), k=gk.t, v=gv.t, seq_stride=16 * tmax * 32, out=out.t, ldo=ldo,
             row_len=dev(np.int32(lens)), row_len_host=np.int32(lens), len_add=len_add)
    if seqs is not None:
        f.update(row_seq=dev(np.int32(seqs)), row_seq_host=np.int32(seqs))
    if skip is not None:
        assert len(skip) == nseq
        f.update(row_skip=dev(np.uint8(skip)))
    if tiles is not None:
        f.update(tiles=dev(np.int32(tiles)), tiles_host=np.int32(tiles), ntiles=len(tiles))
    ran = E().debug_attn(form, **f)
    o = out.np((rows, ldo))
    assert same_bits(gk.np(), K.reshape(-1)) and same_bits(gv.np(), V.reshape(-1)), "a cache was written"
    return o, ran


def split_tiles(spans, cap, ragged=None):
    """Tiles {seq, row0, nrows} of at most cap rows over spans [(seq, row0, nrows)]; ragged: the last
    span's last tile has that many rows."""
    tiles = []
    for i, (s, r0, n) in enumerate(spans):
        tail = ragged if ragged and i == len(spans) - 1 else 0
        body = n - tail
        tiles += [[s, r0 + o, min(cap, body - o)] for o in range(0, body, cap)]
        if tail:
            tiles.append([s, r0 + body, tail])
    return tiles


def check_rows(what, got, ref, lens, fam, kernel, live=None):
    """Every live row within the bar of its own length; returns the worst error / bar."""
    mode, margin = O.BAR_MODE[kernel], O.KERNEL_MARGIN[kernel]
    worst = 0.0
    for r, T in enumerate(lens):
        if live is not None and not live[r]:
            assert np.all(got[r] == SENT), f"{what}: skipped row {r} was written"
            continue
        assert np.all(np.isfinite(got[r])), (what, r)
        err, bar = float(np.abs(got[r].astype(np.float64) - ref[r]).max()), fam.bar(int(T), mode, margin)
        worst = max(worst, err / bar)
        assert err <= bar, f"{what}: row {r} (len {T}) error {err:.3g} above its bar {bar:.3g}"
    print(f"RHO {what}: worst error / bar {worst:.3g}; bars {min(fam.bar(int(T), mode, margin) for T in lens):.3g} .. "
          f"{max(fam.bar(int(T), mode, margin) for T in lens):.3g}")
    return worst


def edge_lens(T):
    """Five rows around a length edge: the edge, one and seven below it, one key, the edge again."""
    return [T, max(T - 1, 1), max(T - 7, 1), 1, T]


def tmax_for(T):
    return TMAX if T <= TMAX else TLONG


@functools.lru_cache(maxsize=None)
def edge_ref(fam, T):
    lens = edge_lens(T)
    q, K, V = caches(fam, 5, 1, tmax_for(T), [T])
    return O.attn_rows(q, K[0], V[0], lens)


def launch_edge(kernel, fam, T, stale=0.0):
    lens = edge_lens(T)
    q, K, V = caches(fam, 5, 1, tmax_for(T), [T], stale)
    if kernel == "rows_plus":      # attn_rows_plus: the lengths arrive one short
        return run_attn("rows", q, K, V, [l - 1 for l in lens], len_add=1)[0]
    tiles = [[0, 0, 5]] if kernel in ("rowlane", "mf32") else None
    return run_attn(kernel, q, K, V, lens, tiles=tiles)[0]


# ------------------------------------------------------------------ lengths at each kernel's edges
@pytest.mark.parametrize("kernel,T", [("rows", T) for T in LENS_ROWS] + [("flash", T) for T in LENS_FLASH] +
                         [("rowlane", T) for T in LENS_FLASH] + [("mf32", T) for T in LENS_MF32])
def test_attention_length_edges(kernel, T):
    got = launch_edge(kernel, O.UNIT, T)
    check_rows(f"{kernel} T={T}", got, edge_ref(O.UNIT, T), edge_lens(T), O.UNIT, kernel)
    if kernel == "rows":
        assert same_bits(launch_edge("rows_plus", O.UNIT, T), got), "attn_rows_plus(len - 1, 1) differs"


@pytest.mark.parametrize("kernel", ("rows",) + PREFILL)
@pytest.mark.parametrize("T", LENS_PEAKED)
def test_attention_peaked(kernel, T):
    """Scores reach tens: a missing max subtraction overflows, a missing rescale fails the bar."""
    got = launch_edge(kernel, O.PEAKED, T)
    check_rows(f"{kernel} peaked T={T}", got, edge_ref(O.PEAKED, T), edge_lens(T), O.PEAKED, kernel)


def test_attn_rows_takes_the_form_its_rule_names():
    q, K, V = caches(O.UNIT, 5, 1, TMAX, [193])
    lens = edge_lens(193)
    auto, ran = run_attn("auto", q, K, V, lens)
    want = auto_form()                                    # k_attn_flash unless GENIE_ATTN_FLASH=0
    assert ran == want and same_bits(auto, run_attn(want, q, K, V, lens)[0])
    for f in (dict(skip=[0]), dict(seqs=[0] * 5)):
        auto, ran = run_attn("auto", q, K, V, lens, **f)
        assert ran == "rows" and same_bits(auto, run_attn("rows", q, K, V, lens)[0])


# ------------------------------------------------------------------ causal tiles of one sequence
L_TEXT, N_CAUSAL = 70, 90
CAUSAL_LENS = [L_TEXT] * L_TEXT + [L_TEXT + 1 + i for i in range(N_CAUSAL)]


@functools.lru_cache(maxsize=None)
def causal_case():
    q, K, V = caches(O.UNIT, len(CAUSAL_LENS), 1, TMAX, [max(CAUSAL_LENS)])
    return q, K, V, O.attn_rows(q, K[0], V[0], CAUSAL_LENS)


@functools.lru_cache(maxsize=None)
def causal_flash():
    q, K, V, _ = causal_case()
    return run_attn("flash", q, K, V, CAUSAL_LENS)[0]


@pytest.mark.parametrize("kernel,ragged", [(k, r) for k in PREFILL for r in (None, 1, 31, 33) if not r or r <= CAP[k]])
def test_causal_tiles(kernel, ragged):
    """70 text rows and 90 causal rows of one sequence: within a tile the waves see different
    longest lengths and skip different chunks.  Every tiling gives k_attn_flash's own rows (a
    k_attn_flash tile holds 16 rows: its ragged tile is the 1-row one)."""
    q, K, V, ref = causal_case()
    tiles = split_tiles([(0, 0, len(CAUSAL_LENS))], CAP[kernel], ragged)
    got = run_attn(kernel, q, K, V, CAUSAL_LENS, tiles=tiles)[0]
    check_rows(f"{kernel} causal tiles ragged={ragged}", got, ref, CAUSAL_LENS, O.UNIT, kernel)
    assert same_bits(got, causal_flash()), f"{kernel}: a row differs from k_attn_flash's"


# ------------------------------------------------------------------ packed prefill
PACKED = [(1, 1), (5, 3), (100, 60)]      # (text rows, causal rows) of three sequences


def packed_layout():
    lens, seqs, spans, r0 = [], [], [], 0
    for s, (L, P) in enumerate(PACKED):
        lens += [L] * L + [L + 1 + i for i in range(P)]
        seqs += [s] * (L + P)
        spans.append((s, r0, L + P))
        r0 += L + P
    return lens, seqs, spans


def packed_case(stale=0.0):
    """Three sequences and a fourth cache that no row addresses."""
    lens, seqs, spans = packed_layout()
    longest = [L + P for L, P in PACKED] + [0]
    return caches(O.UNIT, len(lens), 4, TMAX, longest, stale) + (lens, seqs, spans)


@functools.lru_cache(maxsize=None)
def packed_ref():
    q, K, V, lens, seqs, spans = packed_case()
    return np.concatenate([O.attn_rows(q[r0:r0 + n], K[s], V[s], lens[r0:r0 + n]) for s, r0, n in spans])


def run_packed(kernel, stale=0.0):
    q, K, V, lens, seqs, spans = packed_case(stale)
    if kernel == "rows":
        return run_attn("rows", q, K, V, lens, seqs=seqs)[0]
    return run_attn(kernel, q, K, V, lens, tiles=split_tiles(spans, CAP[kernel]))[0]


@pytest.mark.parametrize("kernel", ("rows",) + PREFILL)
def test_packed_prefill(kernel):
    """A row of a packed launch is the row of its sequence launched alone, bit for bit."""
    q, K, V, lens, seqs, spans = packed_case()
    got = run_packed(kernel)
    check_rows(f"{kernel} packed", got, packed_ref(), lens, O.UNIT, kernel)
    for s, r0, n in spans:
        tiles = split_tiles([(0, 0, n)], CAP[kernel]) if kernel != "rows" else None
        alone = run_attn(kernel, q[r0:r0 + n], K[s:s + 1], V[s:s + 1], lens[r0:r0 + n], tiles=tiles)[0]
        assert same_bits(alone, got[r0:r0 + n]), f"{kernel}: sequence {s} differs from its own launch"


# ------------------------------------------------------------------ stale cache rows, skips, repeats
@pytest.mark.parametrize("kernel", ("rows",) + PREFILL)
def test_stale_cache_rows_are_never_weighted(kernel):
    """NaN at and past every sequence's longest visible length, and all over an unaddressed cache."""
    for got, zero in ((run_packed(kernel, np.nan), run_packed(kernel)),
                      (launch_edge(kernel, O.UNIT, 129, np.nan), launch_edge(kernel, O.UNIT, 129)),
                      (launch_edge(kernel, O.UNIT, 1, np.nan), launch_edge(kernel, O.UNIT, 1))):
        assert np.all(np.isfinite(got)) and same_bits(got, zero)


def test_row_skip_leaves_the_rows_of_a_finished_sequence():
    q, K, V, lens, seqs, spans = packed_case()
    skip = [0, 1, 0, 1]
    got = run_attn("rows", q, K, V, lens, seqs=seqs, skip=skip)[0]
    live = [not skip[s] for s in seqs]
    check_rows("rows row_skip", got, packed_ref(), lens, O.UNIT, "rows", live)
    assert same_bits(got[live], run_packed("rows")[live])


@pytest.mark.parametrize("kernel", ("rows",) + PREFILL)
def test_two_launches_are_equal(kernel):
    assert same_bits(run_packed(kernel), run_packed(kernel))
    assert same_bits(launch_edge(kernel, O.PEAKED, 513), launch_edge(kernel, O.PEAKED, 513))


@pytest.mark.parametrize("T", [193, 257])
def test_rowlane_and_mf32_rows_are_flash_rows(T):
    flash = launch_edge("flash", O.UNIT, T)
    for kernel in ("rowlane", "mf32"):
        assert same_bits(launch_edge(kernel, O.UNIT, T), flash), f"{kernel} T={T}: a row differs from k_attn_flash's"
    peaked = launch_edge("flash", O.PEAKED, T)
    for kernel in ("rowlane", "mf32"):
        assert same_bits(launch_edge(kernel, O.PEAKED, T), peaked), f"{kernel} peaked T={T}"


def test_unclaimed_comparisons_are_recorded():
    """k_attn_rows against k_attn_flash is not claimed equal: the distance is printed for NUMERICS.md
    and only the bars (above) are asserted."""
    for T in (65, 193, 513):
        a, b = launch_edge("rows", O.UNIT, T), launch_edge("flash", O.UNIT, T)
        print(f"RHO rows vs flash T={T}: equal {same_bits(a, b)}, max |diff| {np.abs(a - b).max():.3g}")


# ------------------------------------------------------------------ dec_slabs
def slab_sum(slabs, b_in):
    """b_in + (((s0 + s1) + s2) + ...) in fp32: the prologue has additions only."""
    v = slabs[0].copy()
    for z in range(1, slabs.shape[0]):
        v = v + slabs[z]
    return (b_in[None, :] + v).astype(np.float32)


def dec_case(fam, kvlen, nslab, stale=0.0, seed=0):
    B = len(kvlen)
    tmax = tmax_for(max(kvlen) + 1)
    _, K, V = caches(fam, 1, B, tmax, list(kvlen), stale)
    rng = np.random.default_rng([seed, B, nslab, max(kvlen)])
    slabs = (rng.standard_normal((nslab, B, 1536)) / np.sqrt(nslab)).astype(np.float32)
    slabs[:, :, :1024] *= np.float32(fam.qk)
    b_in = (0.1 * rng.standard_normal(1536)).astype(np.float32)
    return K, V, slabs, b_in


def run_dec(K, V, slabs, b_in, kvlen, done, pad=0):
    """One attn_decode_slabs launch; the slabs lie slab_stride = B * 1536 + pad apart.  Returns out
    [B][512] and the caches after."""
    nslab, B, _ = slabs.shape
    tmax = K.shape[2]
    stride = B * 1536 + pad
    sl = np.full((nslab, stride), SENT, np.float32)
    sl[:, :B * 1536] = slabs.reshape(nslab, -1)
    gk, gv, out = Guard(K.size, K), Guard(V.size, V), Guard(B * 512)
    ran = E().debug_attn("dec_slabs", rows=B, tmax=tmax, k=gk.t, v=gv.t, seq_stride=16 * tmax * 32, out=out.t,
                         row_len=dev(np.int32(kvlen)), row_len_host=np.int32(kvlen), row_skip=dev(np.uint8(done)),
                         slabs=dev(sl), nslab=nslab, slab_stride=stride, b_in=dev(b_in))
    assert ran == "dec_slabs"
    return out.np((B, 512)), gk.np(K.shape), gv.np(V.shape)


def check_dec(what, fam, kvlen, nslab, done=None, pad=0, stale=0.0):
    B = len(kvlen)
    done = [0] * B if done is None else done
    K, V, slabs, b_in = dec_case(fam, kvlen, nslab, stale)
    out, K1, V1 = run_dec(K, V, slabs, b_in, kvlen, done, pad)
    qkv = slab_sum(slabs, b_in)
    Kx, Vx = K.copy(), V.copy()
    ref = np.zeros((B, 512))
    for b in range(B):
        if done[b]:
            continue
        Kx[b, :, kvlen[b]], Vx[b, :, kvlen[b]] = qkv[b, 512:1024].reshape(16, 32), qkv[b, 1024:].reshape(16, 32)
        ref[b] = O.attn_rows(qkv[b:b + 1, :512], Kx[b], Vx[b], [kvlen[b] + 1])[0]
    # the appended rows are the fp32 sum bit for bit, written at kvlen[b] and nowhere else
    assert same_bits(K1, Kx) and same_bits(V1, Vx), f"{what}: the caches are not the old ones plus the new row"
    check_rows(what, out, ref, [k + 1 for k in kvlen], fam, "dec_slabs", [not d for d in done])
    return out


@pytest.mark.parametrize("T", LENS_ROWS)
def test_dec_slabs_length_edges(T):
    check_dec(f"dec_slabs T={T}", O.UNIT, [T - 1, max(T - 2, 0), 0], nslab=4)


@pytest.mark.parametrize("nslab,pad", [(1, 0), (4, 0), (5, 64)])
def test_dec_slabs_prologue_is_the_ordered_sum(nslab, pad):
    check_dec(f"dec_slabs nslab={nslab}", O.UNIT, [99, 0, 256, 63, 64], nslab, pad=pad)


def test_dec_slabs_done_peaked_stale_and_repeat():
    kv = [128, 300, 7, 512]
    check_dec("dec_slabs done", O.UNIT, kv, 4, done=[0, 1, 0, 1])
    for T in LENS_PEAKED:
        check_dec(f"dec_slabs peaked T={T}", O.PEAKED, [T - 1, T - 2], 4)
    a = check_dec("dec_slabs", O.UNIT, kv, 4)
    assert same_bits(a, check_dec("dec_slabs again", O.UNIT, kv, 4))
    nan = check_dec("dec_slabs stale", O.UNIT, kv, 4, stale=np.nan)      # NaN past kvlen[b]: the row's own slot too
    assert same_bits(a, nan)
    # not claimed equal to k_attn_rows on the same keys: recorded only
    K, V, slabs, b_in = dec_case(O.UNIT, kv, 4)
    qkv = slab_sum(slabs, b_in)
    for b in range(len(kv)):
        K[b, :, kv[b]], V[b, :, kv[b]] = qkv[b, 512:1024].reshape(16, 32), qkv[b, 1024:].reshape(16, 32)
    rows = run_attn("rows", qkv[:, :512].copy(), K, V, kv, seqs=list(range(len(kv))), len_add=1)[0]
    print(f"RHO dec_slabs vs rows: equal {same_bits(a, rows)}, max |diff| {np.abs(a - rows).max():.3g}")


# ------------------------------------------------------------------ attn_outproj
@functools.lru_cache(maxsize=None)
def wot():
    return O.f16w(np.random.default_rng(11), 512, 512)


def run_attn_out(q, K, V, kvlen, done=None, acc=None):
    """One attn_outproj launch: part [16][B][512], or with acc (int64 [B][600], pre-loaded) the
    accumulators after."""
    B, tmax = len(kvlen), K.shape[2]
    gk, gv = Guard(K.size, K), Guard(V.size, V)
    f = dict(B=B, tmax=tmax, q=dev(q), k=gk.t, v=gv.t, seq_stride=16 * tmax * 32, kvlen=dev(np.int32(kvlen)),
             kvlen_host=np.int32(kvlen), WoT=dev(wot().astype(np.float16)))
    if done is not None:
        f.update(done=dev(np.uint8(done)))
    if acc is None:
        out = Guard(16 * B * 512)
        f.update(part=out.t)
    else:
        out = Guard(acc.size, acc, dtype=torch.int64, fill=ISENT)
        f.update(acc_out=out.t, acc_bstride=acc.shape[1])
    E().debug_attn_out(**f)
    res = out.np((16, B, 512) if acc is None else acc.shape)
    assert same_bits(gk.np(), K.reshape(-1)) and same_bits(gv.np(), V.reshape(-1)), "a cache was written"
    return res


def check_attn_out(what, fam, kvlen, done=None, stale=0.0):
    B = len(kvlen)
    lens = [k + 1 for k in kvlen]
    q, K, V = caches(fam, B, B, tmax_for(max(lens)), lens, stale)
    part = run_attn_out(q, K, V, kvlen, done)
    margin, worst = O.KERNEL_MARGIN["attn_out"], 0.0
    for b in range(B):
        if done is not None and done[b]:
            assert np.all(part[:, b] == SENT), f"{what}: a finished sequence was written"
            continue
        o = O.attn_row(q[b].reshape(16, 32), K[b], V[b], lens[b])
        ref, S = O.outproj_part64(o, wot())
        # the attention's bar through |WoT|; the 32-term GEMV's bar (4 x the rho of the sequential fp32
        # products of this sequence's own o and WoT, head by head) on S
        W3 = wot().reshape(16, 32, 512)
        bar32 = O.MARGIN * O.group_rho_seq(o.astype(np.float32)[:, None, :], W3)
        tol = fam.bar(lens[b], "f32", margin) * np.abs(W3).sum(1) + bar32 * S
        assert np.all(np.isfinite(part[:, b]))
        worst = max(worst, float((np.abs(part[:, b] - ref) / tol).max()))
    print(f"RHO {what}: worst error / tolerance {worst:.3g}")
    assert worst <= 1.0, what
    return q, K, V, part


@pytest.mark.parametrize("T", LENS_OUT)
def test_attn_out_length_edges(T):
    check_attn_out(f"attn_out T={T}", O.UNIT, [T - 1, max(T - 2, 0), 0])


@pytest.mark.parametrize("B", [1, 3, 8])
def test_attn_out_batches_done_and_fixed_point(B):
    kvlen = [300, 0, 31, 255, 256, 32, 100, 7][:B]
    done = [0, 1, 0, 0, 1, 0, 0, 0][:B]
    q, K, V, part = check_attn_out(f"attn_out B={B}", O.UNIT, kvlen, done if B > 1 else None)
    live = [b for b in range(B) if not (B > 1 and done[b])]
    # the fixed-point path states itself: sum_h rint(double(part) 2^32), all arithmetic shared up to the store
    acc0 = np.full((B, 600), ISENT, np.int64)
    acc0[:, :512] = 5                                    # a pre-loaded accumulator is simply added to
    want = acc0.copy()
    want[live, :512] += O.fx(part[:, live]).sum(0)
    got = run_attn_out(q, K, V, kvlen, done if B > 1 else None, acc0)
    assert np.array_equal(got, want), "acc_out is not the sum of the rounded partials"
    assert np.array_equal(run_attn_out(q, K, V, kvlen, done if B > 1 else None, acc0), want)
    assert same_bits(run_attn_out(q, K, V, kvlen, done if B > 1 else None), part)
    # the hand-off's quantum against the float sum: 16 terms of 2^-33, one fp32 rounding
    s64 = part[:, live].astype(np.float64).sum(0)
    assert np.all(np.abs(O.from_fx(got[live, :512] - 5) - s64) <= 16 * 2.0 ** -33 + 2.0 ** -24 * np.abs(s64))


def test_attn_out_peaked_and_stale():
    for T in LENS_PEAKED:
        check_attn_out(f"attn_out peaked T={T}", O.PEAKED, [T - 1, T - 2])
    kv = [299, 0, 31, 255]
    a = check_attn_out("attn_out", O.UNIT, kv)[3]
    assert same_bits(a, check_attn_out("attn_out stale", O.UNIT, kv, stale=np.nan)[3])


# ------------------------------------------------------------------ gemv_f16
LDC_PAD = 7              # C's rows are N + 7 apart: every sequence's row ends in SENT padding


def gb(rng):
    return (1 + 0.1 * rng.standard_normal(512)).astype(np.float32), (0.1 * rng.standard_normal(512)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gemv_case(N, K):
    return G.Case(8, N, K, seed=3, kind="f16")


def prologue(kind, B, rng):
    """The fields of a prologue and its fp32 pre-LayerNorm rows (None: plain).  B == 3: the rows of
    gemm_oracle.ln_rows, the constant one built from exact sums (0.5 + (0.25 + 0))."""
    if kind == "plain":
        return {}, None
    rows = G.ln_rows(B, 512, rng)
    if kind == "ln_src":
        return dict(src=dev(rows), lds=512), rows
    bias = np.full(512, 0.25, np.float32) if B == 3 else (0.1 * rng.standard_normal(512)).astype(np.float32)
    res = rows.copy()
    n_part = 64 if kind == "ln_part64" else 32
    part = (rng.standard_normal((n_part, B, 512)) / np.sqrt(n_part)).astype(np.float32)
    if B == 3:
        res[1], part[:, 1] = 0.5, 0
    f = dict(part_bias=dev(bias), part_res=dev(res))
    if kind == "ln_acc":
        acc = np.full((B, 520), ISENT, np.int64)
        acc[:, :512] = O.fx(part).sum(0)
        f.update(acc_in=dev(acc), acc_bstride=520)
        return f, (res + (bias[None] + O.from_fx(acc[:, :512]))).astype(np.float32)
    p = np.broadcast_to(bias, (B, 512)).copy()
    for j in range(n_part):                                # fixed order, additions only
        p = p + part[j]
    f.update(part=dev(part), n_part=n_part, part_stride=B * 512)
    return f, (res + p).astype(np.float32)


def run_gemv(N, K, B, kind="plain", mode="store", **kv):
    """One gemv_f16 launch; checks ln_out (LayerNorm prologues) and returns (x the GEMV consumed, C
    [B][ldc], case, the operands of the epilogue)."""
    c = gemv_case(N, K)
    rng = np.random.default_rng([N, K, B, len(kind)])
    f, pre = prologue(kind, B, rng)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    res = rng.standard_normal((B, N)).astype(np.float32)
    ldc = 512 if mode == "qkv" else N + LDC_PAD          # a store past column N lands in checked padding
    C, ln_out = Guard(B * ldc), Guard(B * 512)
    f.update(B=B, N=N, K=K, W=dev(c.W.astype(np.float16)), bias=dev(bias), C=C.t, ldc=ldc)
    if pre is None:
        x = c.A_all[:B]
        f.update(src=dev(x), lds=K)
    else:
        g, b = gb(rng)
        f.update(ln_g=dev(g), ln_b=dev(b), ln_out=ln_out.t)
    if mode == "resid":
        f.update(res=dev(res), ldr=N)
    f.update(kv)
    E().debug_gemv(mode, **f)
    if pre is not None:
        x = ln_out.np((B, 512))
        r, bar = G.ln_rho(x, pre, g, b, O.LN_EPS), O.ln_bar(pre, g, b)
        print(f"RHO gemv {kind} B={B} ln_out: rho_ln {r:.3g} bar {bar:.3g}")
        assert np.all(np.isfinite(x)) and r <= bar, (kind, B, r, bar)
        if B == 3:
            assert np.array_equal(x[1], b), "a constant row is ln_b exactly"
    else:
        assert np.all(ln_out.np() == SENT)
    got = C.np((B, ldc))
    if mode != "qkv":
        assert np.all(got[:, N:] == SENT), "a column at or past N was stored"
        got = got[:, :N]
    return x, got, c, bias, res


def check_gemv(what, x, got, c, bias, mode="store", res=None):
    """C against the fp64 GEMV of the activations the kernel consumed: bar * S and one fp32 rounding
    for the bias add (and one for res + v)."""
    C64, S = G.exact(x, c.W)
    ref = C64 + bias
    tol = c.bar * S + 2.0 ** -24 * np.abs(ref)
    if mode == "relu":
        ref = np.maximum(ref, 0)
    if mode == "resid":
        ref = ref + res
        tol = tol + 2.0 ** -24 * np.abs(ref)
    assert np.all(np.isfinite(got)), what
    q = float((np.abs(got - ref) / tol).max())
    print(f"RHO gemv {what}: worst error / tolerance {q:.3g}, bar {c.bar:.3g}")
    assert q <= 1.0, what


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("N,K", [(1536, 512), (512, 512), (1025, 512), (512, 2048)])
def test_gemv_shapes_and_batches(N, K, B):
    for mode in ("store", "relu", "resid"):
        x, C, c, bias, res = run_gemv(N, K, B, mode=mode)
        check_gemv(f"plain {mode} N={N} K={K} B={B}", x, C, c, bias, mode, res)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("kind", ["ln_src", "ln_part32", "ln_part64", "ln_acc"])
def test_gemv_layernorm_prologues(kind, B):
    """Every NB (1, 2, 4, 8) and a B < NB tail under each prologue; N = 1536 is the two-rows-per-wave form."""
    for N in (512, 1025, 1536):
        x, C, c, bias, res = run_gemv(N, 512, B, kind)
        check_gemv(f"{kind} N={N} B={B}", x, C, c, bias)


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("by_row", [False, True])
def test_gemv_qkv_scatter(B, by_row):
    """q to C, k and v to [(c >> 5) * tmax + pos] * 32 + (c & 31) of the sequence's cache and nowhere else."""
    FILL = 555.5
    pos = [TMAX - 1, 0, 17, 5, 5, 100, 31, 32][:B] if by_row else [17] * B
    skip = [0, 1, 0, 0, 0, 1, 0, 0][:B]
    gk, gv = Guard(B * 16 * TMAX * 32, fill=FILL), Guard(B * 16 * TMAX * 32, fill=FILL)
    kv = dict(kv_k=gk.t, kv_v=gv.t, kv_tmax=TMAX, kv_seq_stride=16 * TMAX * 32, kv_pos0=17)
    if by_row:
        kv.update(kv_row_pos=dev(np.int32(pos)), kv_row_pos_host=np.int32(pos), kv_row_skip=dev(np.uint8(skip)))
    x, C, c, bias, _ = run_gemv(1536, 512, B, "ln_src", "qkv", **kv)
    C64, S = G.exact(x, c.W)
    ref = C64 + bias
    tol = c.bar * S + 2.0 ** -24 * np.abs(ref)
    K1, V1 = gk.np((B, 16, TMAX, 32)), gv.np((B, 16, TMAX, 32))
    got = np.full((B, 1536), np.nan)
    got[:, :512] = C
    for b in range(B):
        live = not (by_row and skip[b])
        for cache, lo in ((K1, 512), (V1, 1024)):
            row = cache[b, :, pos[b]].copy()
            cache[b, :, pos[b]] = FILL
            if live:
                got[b, lo:lo + 512] = row.reshape(512)
            else:
                assert np.all(row == FILL), "a skipped row was scattered"
                got[b, lo:lo + 512] = ref[b, lo:lo + 512]
    assert np.all(K1 == FILL) and np.all(V1 == FILL), "the scatter wrote outside its rows"
    q = float((np.abs(got - ref) / tol).max())
    print(f"RHO gemv qkv B={B} by_row={by_row}: worst error / tolerance {q:.3g}")
    assert q <= 1.0


# ------------------------------------------------------------------ ffn_fused
@functools.lru_cache(maxsize=None)
def ffn_weights():
    c = G.Case(8, 2048, 512, seed=9, kind="f16")
    rng = np.random.default_rng(10)
    W2T = O.f16w(rng, 2048, 512, 1.0 / np.sqrt(2048))
    return c, (0.1 * rng.standard_normal(2048)).astype(np.float32), W2T, (0.1 * rng.standard_normal(512)).astype(np.float32)


def run_ffn(B, nslices, h, attn_part, g, b, fx_in=False, acc0=None):
    c, b1, W2T, bo = ffn_weights()
    h1 = Guard(B * 512)
    f = dict(B=B, nslices=nslices, h=dev(h), bo=dev(bo), ln_g=dev(g), ln_b=dev(b), h1=h1.t, W1=dev(c.W.astype(np.float16)),
             b1=dev(b1), W2T=dev(W2T.astype(np.float16)))
    if fx_in:
        acc = np.full((B, 600), ISENT, np.int64)           # FfnArgs has one acc_bstride for both hand-offs
        acc[:, :512] = O.fx(attn_part).sum(0)
        f.update(acc_attn=dev(acc), acc_bstride=600)
        s1 = (h + (bo[None] + O.from_fx(acc[:, :512]))).astype(np.float32)
    else:
        p = np.broadcast_to(bo, (B, 512)).copy()
        for hh in range(16):
            p = p + attn_part[hh]
        s1 = (h + p).astype(np.float32)
        f.update(attn_part=dev(attn_part))
    if acc0 is None:
        out = Guard(nslices * B * 512)
        f.update(part=out.t)
    else:
        out = Guard(acc0.size, acc0, dtype=torch.int64, fill=ISENT)
        assert acc0.shape[1] == 600
        f.update(acc_out=out.t, acc_bstride=600)
    E().debug_ffn(**f)
    return s1, h1.np((B, 512)), out.np((nslices, B, 512) if acc0 is None else acc0.shape)


@pytest.mark.parametrize("B", [1, 3, 4, 8])
@pytest.mark.parametrize("nslices", [32, 64])
def test_ffn_fused(nslices, B):
    c, b1, W2T, bo = ffn_weights()
    rng = np.random.default_rng([nslices, B])
    h = G.ln_rows(B, 512, rng)
    attn_part = (rng.standard_normal((16, B, 512)) / 4).astype(np.float32)
    g, b = gb(rng)
    for fx_in in (False, True):
        s1, h1, part = run_ffn(B, nslices, h, attn_part, g, b, fx_in)
        r, lbar = G.ln_rho(h1, s1, g, b, O.LN_EPS), O.ln_bar(s1, g, b)
        # the slices from the kernel's own h1: FFN1's bar on S1 and one rounding of the bias add,
        # through relu (1-Lipschitz) and |W2T|; FFN2's bar on S2
        f64, S1, ref, S2, absW = O.ffn_ref(h1, c.W, b1, W2T, nslices)
        tol1 = ((c.bar + 2.0 ** -24) * S1).reshape(B, nslices, -1)
        # FFN2's bar: 4 x the rho of the sequential fp32 products of the case's own f and W2T, slice by slice
        fs = f64.astype(np.float32).reshape(B, nslices, -1).transpose(1, 0, 2)
        bar2 = O.MARGIN * O.group_rho_seq(fs, W2T.reshape(nslices, -1, 512))
        tol = bar2 * S2 + np.einsum("bjr,jrn->jbn", tol1, absW)
        q = float((np.abs(part - ref) / tol).max())
        print(f"RHO ffn nslices={nslices} B={B} fx_in={fx_in}: h1 rho_ln {r:.3g} bar {lbar:.3g}; "
              f"part worst error / tolerance {q:.3g}")
        assert np.all(np.isfinite(h1)) and r <= lbar and np.all(np.isfinite(part)) and q <= 1.0
        # the fixed-point result states itself: sum_j rint(double(part_j) 2^32) on a pre-loaded accumulator
        acc0 = np.full((B, 600), ISENT, np.int64)
        acc0[:, :512] = -3
        want = acc0.copy()
        want[:, :512] += O.fx(part).sum(0)
        for _ in range(2):
            s1b, h1b, acc = run_ffn(B, nslices, h, attn_part, g, b, fx_in, acc0)
            assert same_bits(h1b, h1) and np.array_equal(acc, want), "acc_out is not the sum of the rounded partials"
        assert same_bits(run_ffn(B, nslices, h, attn_part, g, b, fx_in)[2], part)


# ------------------------------------------------------------------ embeds
def sum_or_fma(got, e, al, pe, what):
    """e + al * pe in fp32 as numpy rounds it (product, then sum), or with the product contracted into
    an fma (the exact product added and rounded once; the device may do either).  One ulp between the
    two is the usual case but not a bound: where e and al * pe cancel, the product's own rounding is
    worth several ulps of the sum, so each element is held to one of the two values."""
    two = e + al * pe
    exact = e.astype(np.float64) + np.float64(al) * pe.astype(np.float64)
    fma = np.abs(got.astype(np.float64) - exact) <= 0.5 * np.spacing(np.abs(got)).astype(np.float64)
    assert got.dtype == np.float32 and two.dtype == np.float32
    assert np.all((got == two) | fma), what
    assert np.all(np.abs(got.astype(np.float64) - two) <= np.spacing(np.abs(two)) + 0.5 * np.spacing(np.abs(al * pe))), what


def test_embeds():
    rng = np.random.default_rng(21)
    emb = G.f16(rng.standard_normal((1025, 512)))
    pe = rng.standard_normal((40, 512)).astype(np.float32)
    alpha = np.float32([0.3712])
    common = dict(emb=dev(emb), alpha=dev(alpha), pe=dev(pe), n_tok=1025, n_pe=40)
    B, ldy = 5, 12
    y = rng.integers(0, 1025, (B, ldy)).astype(np.int64)
    ny = np.int32([1, 12, 7, 3, 9])
    y[1, 11], y[0, 0] = 1024, 0
    done = np.uint8([0, 0, 1, 0, 0])
    out = Guard(B * 512)
    E().debug_embed("decode_embed", n=B, tok=dev(y), tok_host=y, ldy=ldy, ny=dev(ny), ny_host=ny, out=out.t,
                    done=dev(done), **common)
    o = out.np((B, 512))
    tok = y[np.arange(B), ny - 1]
    live = done == 0
    assert np.all(o[2] == SENT), "a finished sequence was written"
    sum_or_fma(o[live], emb[tok].astype(np.float32)[live], alpha[0], pe[ny][live], "decode_embed")
    P = 9
    toks = np.int64([1024, 0, 5, 5, 77, 1000, 512, 3, 1023])
    out = Guard(P * 512)
    E().debug_embed("audio_embed_prompts", n=P, tok=dev(toks), tok_host=toks, out=out.t, **common)
    sum_or_fma(out.np((P, 512)), emb[toks].astype(np.float32), alpha[0], pe[1:P + 1], "audio_embed_prompts")


@pytest.mark.parametrize("n_ssl", [1, 2, 7, 8])
def test_ssl_im2col_is_exact(n_ssl):
    ssl = np.random.default_rng(n_ssl).standard_normal((768, n_ssl)).astype(np.float32)
    P = n_ssl // 2                                          # an odd count drops the last frame
    out = Guard(max(P, 1) * 1536)
    E().debug_embed("ssl_im2col", n=n_ssl, ssl=dev(ssl), out=out.t)
    o = out.np((max(P, 1), 1536))
    if P == 0:
        assert np.all(o == SENT)
        return
    ref = ssl[:, :2 * P].reshape(768, P, 2).transpose(1, 0, 2).reshape(P, 1536)
    assert np.array_equal(o, ref)
