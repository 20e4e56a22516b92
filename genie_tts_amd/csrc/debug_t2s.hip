// Engine-free debug hooks (tests only) for the T2S decoder's own kernels: the prefill attention
// kernels, the batched decode attention, the three fused launches of the B <= 8 decode step and the
// exact embedding kernels.  Each launches one kernel from a flat description and checks its
// arguments against what the kernel loads and stores before any HIP call (debug_gemm.hip's rules).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <string>

#include "../../include/genie_engine.h"
#include "engine_internal.h"
#include "kernels.h"
#include "prefill_attn.h"

using namespace gsv;

namespace {

constexpr int ATTN_LDS_KEYS = 4096;   // ATTN_MAXT (t2s.hip): the LDS score array of k_attn_rows / k_attn_dec_slabs
enum { F_AUTO = 0, F_ROWS = 1, F_FLASH = 2, F_ROWLANE = 3, F_MF32 = 4, F_DEC = 5 };

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int bad(const char* hook, const std::string& msg) { return set_error(GSV_E_ARG, std::string("debug ") + hook + ": " + msg); }

int launched(const char* what) {
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? 0 : hip_error(what, le);
}

// 0, or GSV_E_ARG: everything the attention kernels assume of their arguments
int attn_check(const gsv_attn_desc* d) {
    auto no = [](const std::string& m) { return bad("attn", m); };
    if (!d) return no("null description");
    if (d->form < F_AUTO || d->form > F_DEC) return no("form: 0 .. 5");
    if (d->rows <= 0 || d->tmax <= 0) return no("rows and tmax must be positive");
    const bool dec = d->form == F_DEC;
    if (!d->k || !d->v || !d->out) return no("null k, v or out");
    if (!dec && !d->q) return no("null q");
    if (!d->row_len || !d->row_len_host) return no(dec ? "null kvlen (row_len and its host copy)" : "null row_len (and its host copy)");
    if (d->form != F_ROWS && d->len_add != 0) return no("len_add is attn_rows_plus's");
    if (!al16(d->k) || !al16(d->v) || (!dec && !al16(d->q))) return no("q, k and v must be 16-B aligned");
    if (!dec && (d->ldq % 4 != 0 || d->ldq < 512)) return no("ldq must be a multiple of 4 and at least 512");
    if (!dec && d->ldo < 512) return no("ldo below 512");
    if (d->seq_stride % 4 != 0) return no("seq_stride must be a multiple of 4");
    const int add = dec ? 1 : d->len_add;
    const bool lds = d->form == F_ROWS || dec;
    for (int r = 0; r < d->rows; ++r) {
        const int64_t len = (int64_t)d->row_len_host[r] + add;
        if (len < 1 || len > d->tmax) return no(dec ? "kvlen[b] + 1 outside [1, tmax]" : "a row's length outside [1, tmax]");
        if (lds && len > ATTN_LDS_KEYS) return no("a length above 4096 (the LDS score array)");
    }
    int nseq = 1;
    if (d->row_seq) {
        if (!d->row_seq_host) return no("row_seq needs its host copy");
        for (int r = 0; r < d->rows; ++r) {
            if (d->row_seq_host[r] < 0) return no("a row names a sequence < 0");
            nseq = d->row_seq_host[r] + 1 > nseq ? d->row_seq_host[r] + 1 : nseq;
        }
    }
    if (dec) {
        nseq = d->rows;
        if (d->rows > 65535) return no("B above the grid's y extent");
        if (d->nslab < 1) return no("nslab must be at least 1");
        if (!d->slabs || !d->b_in) return no("null slabs or b_in");
        if (!d->row_skip) return no("null done (row_skip)");
        if (d->row_seq || d->tiles) return no("dec_slabs takes no row_seq and no tiles");
        if (d->nslab > 1 && d->slab_stride < (int64_t)d->rows * 1536) return no("slabs overlap");
    }
    const bool tiled = d->form == F_ROWLANE || d->form == F_MF32;
    if (tiled && !d->tiles) return no("rowlane and mf32 run over a tile table");
    if (d->tiles) {
        if (d->form == F_AUTO || d->form == F_ROWS) return no("attn_rows takes no tile table");
        if (!d->tiles_host || d->ntiles <= 0 || d->ntiles > 65535) return no("tiles need their host copy and ntiles in [1, 65535]");
        const int cap = d->form == F_FLASH ? 16 : d->form == F_ROWLANE ? 64 * ROWLANE_NW : 32 * MF32_NW;
        for (int t = 0; t < d->ntiles; ++t) {
            const int32_t* tl = d->tiles_host + 3 * t;
            if (tl[0] < 0) return no("a tile names a sequence < 0");
            if (tl[2] < 1 || tl[2] > cap) return no("a tile's rows outside what a block holds");
            if (tl[1] < 0 || (int64_t)tl[1] + tl[2] > d->rows) return no("a tile runs past rows");
            nseq = tl[0] + 1 > nseq ? tl[0] + 1 : nseq;
        }
    }
    if (d->form != F_AUTO && d->form != F_ROWS && !dec && (d->row_seq || d->row_skip))
        return no("flash, rowlane and mf32 read neither row_seq nor row_skip");
    // the grid's y extent of the kernel that is launched: a block per row (k_attn_rows) or per 16 rows
    // (k_attn_flash without tiles); a tile table's ntiles is bounded above
    {
        int form = d->form;
        if (form == F_AUTO) {
            AttnArgs a{};
            a.row_seq = d->row_seq; a.row_skip = d->row_skip;
            form = (int)attn_form(a, attn_flash_enabled());
        }
        const int64_t gy = form == F_ROWS ? d->rows : form == F_FLASH && !d->tiles ? ((int64_t)d->rows + 15) / 16 : 0;
        if (gy > 65535) return no("rows above the grid's y extent");
    }
    if (tiled && (d->ldo % 4 != 0 || !al16(d->out))) return no("rowlane and mf32 store float4: ldo % 4 == 0 and out 16-B aligned");
    if (nseq > 1 && d->seq_stride < (int64_t)16 * d->tmax * 32) return no("seq_stride below one cache");
    return 0;
}

AttnArgs attn_args(const gsv_attn_desc* d) {
    AttnArgs a{};
    a.q = d->q; a.ldq = d->ldq; a.k = d->k; a.v = d->v; a.seq_stride = d->seq_stride; a.tmax = d->tmax;
    a.row_len = d->row_len; a.row_seq = d->row_seq; a.out = d->out; a.ldo = d->ldo; a.rows = d->rows;
    a.scale = d->scale; a.row_skip = d->row_skip; a.tiles = d->tiles; a.ntiles = d->tiles ? d->ntiles : 0;
    return a;
}

}  // namespace

extern "C" int gsv_debug_attn(const gsv_attn_desc* d, void* stream, int32_t* form) {
    if (!form) return bad("attn", "null form");
    *form = -1;
    if (int e = attn_check(d)) return e;
    const AttnArgs a = attn_args(d);
    *form = d->form == F_AUTO ? (int32_t)attn_form(a, attn_flash_enabled()) : d->form;
    if (d->dry) return 0;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    switch (d->form) {
        case F_AUTO: attn_rows(a, s); break;
        case F_ROWS: attn_rows_plus(a, d->len_add, s); break;
        case F_FLASH: attn_rows_flash(a, s); break;
        case F_ROWLANE: attn_rows_rowlane(a, s); break;
        case F_MF32: attn_rows_mf32(a, s); break;
        default: {
            AttnDecArgs x{};
            x.slabs = d->slabs; x.nslab = d->nslab; x.slab_stride = d->slab_stride; x.b_in = d->b_in;
            x.k = d->k; x.v = d->v; x.seq_stride = d->seq_stride; x.tmax = d->tmax;
            x.kvlen = d->row_len; x.done = d->row_skip; x.out = d->out; x.B = d->rows; x.scale = d->scale;
            attn_decode_slabs(x, s);
        }
    }
    return launched("debug attn launch");
}

extern "C" int gsv_debug_attn_out(const gsv_attn_out_desc* d, void* stream) {
    auto no = [](const std::string& m) { return bad("attn_out", m); };
    if (!d) return no("null description");
    if (d->B <= 0 || d->B > 65535 || d->tmax <= 0) return no("B (up to 65535) and tmax must be positive");
    if (!d->q || !d->k || !d->v || !d->WoT || !d->kvlen || !d->kvlen_host) return no("null q, k, v, WoT or kvlen (and its host copy)");
    if (!al16(d->q) || !al16(d->k) || !al16(d->v) || !al16(d->WoT)) return no("q, k, v and WoT must be 16-B aligned");
    if ((d->part != nullptr) == (d->acc_out != nullptr)) return no("exactly one of part and acc_out");
    if (d->seq_stride % 4 != 0) return no("seq_stride must be a multiple of 4");
    if (d->B > 1 && d->seq_stride < (int64_t)16 * d->tmax * 32) return no("seq_stride below one cache");
    if (d->acc_out && d->B > 1 && d->acc_bstride < 512) return no("acc_bstride below 512");
    for (int b = 0; b < d->B; ++b)
        if (d->kvlen_host[b] < 0 || (int64_t)d->kvlen_host[b] + 1 > d->tmax) return no("kvlen[b] + 1 outside [1, tmax]");
    AttnOutArgs a{};
    a.B = d->B; a.q = d->q; a.k = d->k; a.v = d->v; a.seq_stride = d->seq_stride; a.tmax = d->tmax;
    a.kvlen = d->kvlen; a.done = d->done; a.scale = d->scale; a.WoT = reinterpret_cast<const __half*>(d->WoT);
    a.part = d->part; a.acc_out = reinterpret_cast<long long*>(d->acc_out); a.acc_bstride = d->acc_bstride;
    (void)hipGetLastError();
    attn_outproj(a, (hipStream_t)stream);
    return launched("debug attn_out launch");
}

extern "C" int gsv_debug_gemv(const gsv_gemv_desc* d, void* stream) {
    auto no = [](const std::string& m) { return bad("gemv", m); };
    if (!d) return no("null description");
    // NB = 1, 2, 4, 8 sequences of LDS: a ninth would be written past it (plain) or dropped (LayerNorm)
    if (d->B < 1 || d->B > 8) return no("B outside [1, 8]");
    if (d->K != 512 && d->K != 2048) return no("K: 512 or 2048");
    if (d->N <= 0) return no("N must be positive");
    if (d->mode < EPI_STORE || d->mode > EPI_QKV) return no("mode: store, relu, resid or qkv");
    if (d->ln_g && d->K != 512) return no("the LayerNorm prologue is K = 512");
    if (d->ln_g && !d->ln_b) return no("ln_g without ln_b");
    if (!d->ln_g && (d->part || d->acc_in)) return no("part / acc_in are read by the LayerNorm prologue only");
    if (d->part && d->acc_in) return no("both part and acc_in");
    if (d->part && (d->n_part <= 0 || d->n_part % 16 != 0)) return no("n_part must be a positive multiple of 16");
    if ((d->part || d->acc_in) && (!d->part_bias || !d->part_res)) return no("part / acc_in need part_bias and part_res");
    if (d->part && d->part_stride < (int64_t)d->B * 512 && d->n_part > 1) return no("partials overlap");
    if (d->acc_in && d->B > 1 && d->acc_bstride < 512) return no("acc_bstride below 512");
    if (!d->part && !d->acc_in) {
        if (!d->src) return no("null src");
        if (d->lds < d->K) return no("lds below K");
        if (!d->ln_g && (d->lds % 4 != 0 || !al16(d->src))) return no("the plain prologue needs lds % 4 == 0 and src 16-B aligned");
    }
    if (!d->W || !al16(d->W)) return no("W must be non-null and 16-B aligned");
    if (!d->C) return no("null C");
    if (d->mode != EPI_QKV && d->ldc < d->N) return no("ldc below N");
    if (d->mode == EPI_RESID && (!d->res || d->ldr < d->N)) return no("EPI_RESID needs res with ldr >= N");
    if (d->mode == EPI_QKV) {
        if (d->N != 1536 || d->ldc < 512) return no("EPI_QKV needs N == 1536 and ldc >= 512");
        if (!d->kv_k || !d->kv_v || d->kv_tmax <= 0) return no("EPI_QKV needs the K/V caches and tmax");
        if (d->B > 1 && d->kv_seq_stride < (int64_t)16 * d->kv_tmax * 32) return no("seq_stride below one cache");
        if (d->kv_row_pos && !d->kv_row_pos_host) return no("kv_row_pos needs its host copy");
        for (int b = 0; b < d->B; ++b) {
            const int pos = d->kv_row_pos ? d->kv_row_pos_host[b] : d->kv_pos0;
            if (pos < 0 || pos >= d->kv_tmax) return no("a position past tmax");
        }
    }
    GemvArgs a{};
    a.B = d->B; a.N = d->N; a.K = d->K; a.src = d->src; a.lds = d->lds;
    a.part = d->part; a.n_part = d->n_part; a.part_stride = d->part_stride; a.part_bias = d->part_bias; a.part_res = d->part_res;
    a.ln_g = d->ln_g; a.ln_b = d->ln_b; a.ln_out = d->ln_out;
    a.W = reinterpret_cast<const __half*>(d->W); a.bias = d->bias; a.C = d->C; a.ldc = d->ldc; a.mode = d->mode;
    a.res = d->res; a.ldr = d->ldr;
    a.kv.k = d->kv_k; a.kv.v = d->kv_v; a.kv.tmax = d->kv_tmax; a.kv.pos0 = d->kv_pos0; a.kv.row_pos = d->kv_row_pos;
    a.kv.seq_stride = d->kv_seq_stride; a.kv.row_skip = d->kv_row_skip;
    a.acc_in = reinterpret_cast<const long long*>(d->acc_in); a.acc_bstride = d->acc_bstride;
    (void)hipGetLastError();
    gemv_f16(a, (hipStream_t)stream);
    return launched("debug gemv launch");
}

extern "C" int gsv_debug_ffn(const gsv_ffn_desc* d, void* stream) {
    auto no = [](const std::string& m) { return bad("ffn", m); };
    if (!d) return no("null description");
    if (d->nslices != 32 && d->nslices != 64) return no("nslices: 32 or 64");
    if (d->B < 1 || d->B > 8) return no("B outside [1, 8]");
    if (!d->h || !d->bo || !d->ln_g || !d->ln_b || !d->h1 || !d->W1 || !d->b1 || !d->W2T) return no("null tensor");
    if ((d->attn_part != nullptr) == (d->acc_attn != nullptr)) return no("exactly one of attn_part and acc_attn");
    if ((d->part != nullptr) == (d->acc_out != nullptr)) return no("exactly one of part and acc_out");
    if (!al16(d->W1) || !al16(d->W2T)) return no("W1 and W2T must be 16-B aligned");
    if ((d->acc_attn || d->acc_out) && d->B > 1 && d->acc_bstride < 512) return no("acc_bstride below 512");
    FfnArgs a{};
    a.B = d->B; a.nslices = d->nslices; a.h = d->h; a.bo = d->bo; a.attn_part = d->attn_part;
    a.ln_g = d->ln_g; a.ln_b = d->ln_b; a.h1 = d->h1;
    a.W1 = reinterpret_cast<const __half*>(d->W1); a.b1 = d->b1; a.W2T = reinterpret_cast<const __half*>(d->W2T);
    a.part = d->part; a.acc_attn = reinterpret_cast<const long long*>(d->acc_attn);
    a.acc_out = reinterpret_cast<long long*>(d->acc_out); a.acc_bstride = d->acc_bstride;
    (void)hipGetLastError();
    ffn_fused(a, (hipStream_t)stream);
    return launched("debug ffn launch");
}

extern "C" int gsv_debug_embed(const gsv_embed_desc* d, void* stream) {
    auto no = [](const std::string& m) { return bad("embed", m); };
    if (!d) return no("null description");
    if (d->op < 0 || d->op > 2) return no("op: 0 .. 2");
    if (d->n <= 0 || d->n > 65535) return no("n outside [1, 65535]");
    if (!d->out) return no("null out");
    hipStream_t s = (hipStream_t)stream;
    if (d->op == 2) {
        if (!d->ssl) return no("null ssl");
        (void)hipGetLastError();
        ssl_im2col(d->ssl, d->n, d->out, s);
        return launched("debug embed launch");
    }
    if (!d->tok || !d->tok_host || !d->emb || !d->alpha || !d->pe) return no("null tok (or its host copy), emb, alpha or pe");
    if (d->n_tok <= 0 || d->n_pe <= 0) return no("n_tok and n_pe must be positive");
    if (d->op == 0) {
        if (!d->ny || !d->ny_host || d->ldy <= 0) return no("decode_embed needs ny (and its host copy) and ldy");
        for (int b = 0; b < d->n; ++b) {
            const int n = d->ny_host[b];
            if (n < 1 || n > d->ldy) return no("ny[b] outside [1, ldy]");
            if (n >= d->n_pe) return no("a pe row past n_pe");
            const int64_t t = d->tok_host[(int64_t)b * d->ldy + n - 1];
            if (t < 0 || t >= d->n_tok) return no("a token outside the table");
        }
        (void)hipGetLastError();
        decode_embed(d->n, d->tok, d->ldy, d->ny, reinterpret_cast<const __half*>(d->emb), d->alpha, d->pe, d->out,
                     d->done, s);
        return launched("debug embed launch");
    }
    if (d->n + 1 > d->n_pe) return no("a pe row past n_pe");
    for (int p = 0; p < d->n; ++p)
        if (d->tok_host[p] < 0 || d->tok_host[p] >= d->n_tok) return no("a token outside the table");
    (void)hipGetLastError();
    audio_embed_prompts(d->tok, d->n, reinterpret_cast<const __half*>(d->emb), d->alpha, d->pe, d->out, s);
    return launched("debug embed launch");
}
