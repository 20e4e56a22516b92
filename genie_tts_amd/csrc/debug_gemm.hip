// Engine-free debug hooks (tests only) for the GEMM entry and the row kernels around it:
// gsv_debug_gemm launches gemm_nt once from a flat description and reports the form that
// ran (gemm_form, the rule gemm_nt itself switches on); gsv_debug_rows launches one row kernel.
// Both check their arguments against what the kernels load and store before any HIP call.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <string>

#include "../../include/genie_engine.h"
#include "engine_internal.h"
#include "kernels.h"

using namespace gsv;

namespace {

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int bad(const std::string& msg) { return set_error(GSV_E_ARG, "debug gemm: " + msg); }

// 0 and `out` filled, or GSV_E_ARG: everything gemm_nt and its kernels assume of their arguments.
int gemm_args(const gsv_gemm_desc* d, GemmArgs& a) {
    if (!d) return bad("null description");
    if (d->M <= 0 || d->N <= 0 || d->K <= 0) return bad("M, N, K must be positive");
    if (d->w_kind < 0 || d->w_kind > 2) return bad("w_kind: 0 (f32), 1 (f16) or 2 (f16 hi + lo)");
    if (d->mode < EPI_STORE || d->mode > EPI_RELU_SPLIT) return bad("unknown mode");
    if (!d->w) return bad("null W");
    if ((d->w_kind == 2) != (d->wl != nullptr)) return bad("the lo plane goes with w_kind 2 and only with it");
    if (!d->a && !(d->ah && d->al)) return bad("null A");
    if ((d->ah != nullptr) != (d->al != nullptr)) return bad("pre-split A needs both planes");
    if (d->lda <= 0 || d->ldw < d->K) return bad("lda must be positive and ldw at least K");
    if (d->mode == EPI_RELU_SPLIT ? (!d->ch || !d->cl) : !d->c) return bad("null C");
    if (d->mode != EPI_QKV && d->ldc < d->N) return bad("ldc below N");
    if (d->small_ns != 0 && (d->small_ns < 2 || d->small_ns > 4)) return bad("small_ns: 0, 2, 3 or 4");
    if (d->cus < 0) return bad("cus must not be negative");
    if (d->a_nslab < 0) return bad("a_nslab must not be negative");

    a = GemmArgs{};
    a.M = d->M; a.N = d->N; a.K = d->K;
    a.A = d->a; a.lda = d->lda;
    a.W = d->w; a.ldw = d->ldw; a.w_f16 = d->w_kind != 0;
    a.Wl = d->wl;
    a.bias = d->bias;
    a.C = d->c; a.ldc = d->ldc;
    a.mode = d->mode;
    a.res = d->res; a.ldr = d->ldr;
    a.rowsq = d->rowsq; a.colsq = d->colsq;
    a.kv.k = d->kv_k; a.kv.v = d->kv_v; a.kv.tmax = d->kv_tmax; a.kv.pos0 = d->kv_pos0;
    a.kv.row_pos = d->kv_row_pos; a.kv.seq_stride = d->kv_seq_stride;
    a.kv.row_seq = d->kv_row_seq; a.kv.row_skip = d->kv_row_skip;
    a.ksplit = d->ksplit; a.slab_stride = d->slab_stride;
    a.a_nslab = d->a_nslab; a.a_slab_stride = d->a_slab_stride; a.a_bias = d->a_bias; a.a_relu = d->a_relu;
    a.Ah = reinterpret_cast<const __half*>(d->ah); a.Al = reinterpret_cast<const __half*>(d->al);
    a.Ch = reinterpret_cast<__half*>(d->ch); a.Cl = reinterpret_cast<__half*>(d->cl);
    a.cus = d->cus; a.small_ns = d->small_ns;

    const GemmForm form = gemm_form(a);
    if (form == GF_BAD_SPLITW)
        return bad("split weights need K % 128 == 0, lda % 4 == 0, ldw % 8 == 0, no A prologue and no EPI_VQDIST");
    if (form == GF_BAD_PRESPLIT) return bad("pre-split A on a shape without the large-M path");
    if (form == GF_BAD_SMALL_NS) return bad("small_ns: 0, 2, 3 or 4");
    // pre-split planes are read by the large-M twin alone: any other kernel would read A instead
    if (d->ah && form != GF_LARGEM_PS) return bad("pre-split A on a shape without the large-M path");
    if (form == GF_LARGEM_PS && (!al16(d->ah) || !al16(d->al))) return bad("pre-split A planes must be 16-B aligned");
    if (form != GF_LARGEM_PS && !d->a) return bad("null A");
    const bool generic = form == GF_GENERIC_F32 || form == GF_GENERIC_F16;
    if (generic) {
        // k_gemm_nt: float4 pairs of A and (f32) W, one uint4 of 8 fp16 weights, in K-steps of 32
        if (d->K % 32 != 0) return bad("the generic kernel needs K % 32 == 0");
        if (d->lda % 4 != 0 || !al16(d->a)) return bad("the generic kernel needs lda % 4 == 0 and A 16-B aligned");
        if (d->ldw % (form == GF_GENERIC_F16 ? 8 : 4) != 0 || !al16(d->w))
            return bad("the generic kernel needs 16-B aligned weight rows (ldw % 4 == 0 for f32, ldw % 8 == 0 for f16)");
        if (d->mode == EPI_SLAB) return bad("EPI_SLAB needs fp16 weights with K % 128 == 0, lda % 4 == 0, ldw % 8 == 0");
        if (d->a_nslab > 0) return bad("an A prologue needs the fp16-weight path (K % 128 == 0, lda % 4 == 0, ldw % 8 == 0)");
    } else {
        // 16-B loads / LDS-DMA of A, W (and Wl) rows; K % 128, lda % 4, ldw % 8 hold by the form
        if (form != GF_LARGEM_PS && !al16(d->a)) return bad("A must be 16-B aligned");
        if (!al16(d->w) || (d->wl && !al16(d->wl))) return bad("weight planes must be 16-B aligned");
    }
    if (d->mode == EPI_SLAB) {
        if (!gemm_slabs_supported(d->K, d->lda, d->ldw)) return bad("EPI_SLAB on an unsupported shape");
        if (d->ksplit < 1 || d->ksplit > 65535) return bad("ksplit must be in [1, 65535]");
        if (d->ksplit > 1 && d->slab_stride < (int64_t)(d->M - 1) * d->ldc + d->N) return bad("slabs overlap");
    }
    if (d->a_nslab > 0) {
        if (form != GF_X2) return bad("an A prologue runs on k_gemm_x2 only");
        if (!d->a_bias || !al16(d->a_bias)) return bad("the A prologue needs a 16-B aligned a_bias");
        if (d->a_nslab > 1 && (d->a_slab_stride <= 0 || d->a_slab_stride % 4 != 0))
            return bad("a_slab_stride must be a positive multiple of 4");
    }
    if (d->mode == EPI_RESID && (!d->res || d->ldr < d->N)) return bad("EPI_RESID needs res with ldr >= N");
    if (d->mode == EPI_VQDIST && (!d->rowsq || !d->colsq)) return bad("EPI_VQDIST needs rowsq and colsq");
    if (d->mode == EPI_QKV) {
        if (d->N != 1536 || d->ldc < 512) return bad("EPI_QKV needs N == 1536 and ldc >= 512");
        if (!d->kv_k || !d->kv_v || d->kv_tmax <= 0) return bad("EPI_QKV needs the K/V caches and tmax");
        if (!d->kv_row_pos && (d->kv_pos0 < 0 || (int64_t)d->kv_pos0 + d->M > d->kv_tmax))
            return bad("EPI_QKV rows run past tmax");
        if (d->kv_row_seq && d->kv_seq_stride < (int64_t)16 * d->kv_tmax * 32) return bad("seq_stride below one cache");
    }
    return 0;
}

int bad_rows(const std::string& msg) { return set_error(GSV_E_ARG, "debug rows: " + msg); }

}  // namespace

extern "C" int gsv_debug_gemm(const gsv_gemm_desc* d, void* stream, int32_t* form) {
    if (!form) return bad("null form");
    *form = -1;
    GemmArgs a;
    if (int e = gemm_args(d, a)) return e;
    *form = (int32_t)gemm_form(a);
    if (d->dry) return 0;
    (void)hipGetLastError();
    gemm_nt(a, (hipStream_t)stream);
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? 0 : hip_error("debug gemm launch", le);
}

extern "C" int gsv_debug_rows(const gsv_rows_desc* d, void* stream) {
    if (!d) return bad_rows("null description");
    if (d->op < 0 || d->op > 5) return bad_rows("op: 0 .. 5");
    if (d->rows < 0) return bad_rows("rows must not be negative");
    if (!d->in || !d->out) return bad_rows("null in / out");
    const bool ln = d->op <= 3, slabs = d->op == 1 || d->op == 3;
    if (ln && (!d->g || !d->b)) return bad_rows("LayerNorm needs g and b");
    if ((d->op == 0 || d->op == 1) && d->D != 512) return bad_rows("layernorm_rows(_slabs) is D = 512");
    if ((d->op == 2 || d->op == 3) && (d->D < 1 || d->D > 1024)) return bad_rows("layernorm_rows_d(_slabs) covers 1 <= D <= 1024");
    if ((d->op == 2 || d->op == 3) && !(d->eps >= 0.f)) return bad_rows("eps must not be negative");
    if (slabs) {
        if (d->nslab < 1 || !d->bias || !d->res) return bad_rows("the slab forms need nslab >= 1, bias and res");
        if (d->nslab > 1 && d->slab_stride < (int64_t)d->rows * d->D) return bad_rows("slabs overlap");
    }
    if (d->op == 1 ? (d->out_hi != nullptr) != (d->out_lo != nullptr) : (d->out_hi || d->out_lo))
        return bad_rows("out_hi / out_lo: both or neither, layernorm_rows_slabs only");
    if (d->op >= 4 && d->D < 1) return bad_rows("cols must be positive");
    if (d->op == 4 && d->ld < d->D) return bad_rows("ld below cols");
    if (d->rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    float* out = reinterpret_cast<float*>(d->out);
    (void)hipGetLastError();
    switch (d->op) {
        case 0: layernorm_rows(d->in, out, d->rows, d->g, d->b, s); break;
        case 1:
            layernorm_rows_slabs(d->in, d->nslab, d->slab_stride, d->bias, d->res, out, d->rows, d->g, d->b, s,
                                 reinterpret_cast<__half*>(d->out_hi), reinterpret_cast<__half*>(d->out_lo));
            break;
        case 2: layernorm_rows_d(d->in, out, d->rows, d->D, d->g, d->b, d->eps, s); break;
        case 3:
            layernorm_rows_d_slabs(d->in, d->nslab, d->slab_stride, d->bias, d->res, out, d->rows, d->D, d->g, d->b,
                                   d->eps, s);
            break;
        case 4: sumsq_rows(d->in, d->ld, d->rows, d->D, out, s); break;
        case 5: argmin_dist_rows(d->in, d->rows, d->D, reinterpret_cast<int64_t*>(d->out), s); break;
    }
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? 0 : hip_error("debug rows launch", le);
}
