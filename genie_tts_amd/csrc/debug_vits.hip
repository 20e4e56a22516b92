// Engine-free debug hooks (tests only) for the vocoder's kernels: gsv_debug_conv launches conv1d /
// conv1d_deferred once from a flat description and reports the form that ran (conv_form, the rule
// conv1d itself switches on); gsv_debug_mrf_pair, gsv_debug_mha and gsv_debug_vits_rows launch the
// fused ResBlock step, the attention and one row kernel.  Each checks its arguments against what
// the kernels load and store before any HIP call.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <string>

#include "../../include/genie_engine.h"
#include "engine_internal.h"
#include "vits.h"

using namespace gsv;

namespace {

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int bad(const char* hook, const std::string& msg) { return set_error(GSV_E_ARG, std::string(hook) + ": " + msg); }

int launched(const char* what) {
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? 0 : hip_error(what, le);
}

// 0 and `a`, `f` filled, or GSV_E_ARG: everything conv1d and its kernels assume of their arguments.
int conv_args(const gsv_conv_desc* d, ConvArgs& a, ConvForm& f) {
    auto no = [](const std::string& m) { return bad("debug conv", m); };
    if (!d) return no("null description");
    if (d->Cin <= 0 || d->Cout <= 0 || d->Tin <= 0 || d->n_t <= 0 || d->o_len <= 0)
        return no("Cin, Cout, Tin, n_t and o_len must be positive");
    if (d->pad < 0 || d->o_tstride < 1 || d->phases < 0) return no("pad, o_tstride >= 1 and phases must not be negative");
    if (d->mode < CV_STORE || d->mode > CV_SPLIT_RESID) return no("unknown mode");
    if (d->dil < 1 || d->dil > 5) return no("dil outside 1 .. 5");
    const bool h = d->wh != nullptr;
    const int K = d->K;
    if (h ? !(K == 1 || K == 2 || K == 3 || K == 4 || K == 7 || K == 11)
          : !(K == 1 || K == 2 || K == 3 || K == 4 || K == 5 || K == 7 || K == 11))
        return no(h ? "K outside the f16 path's instances 1, 2, 3, 4, 7, 11" : "K outside the f32 instances 1, 2, 3, 4, 5, 7, 11");
    if (!d->x) return no("null x");
    if (d->x_cs < 1 || d->x_ts < 1 || d->o_cs < 1 || d->o_ts < 1) return no("x and out strides must be positive");
    if (d->tile_force < 0 || d->tile_force > 4) return no("tile_force: 0 .. 4");
    if (d->ws < 0) return no("ws must not be negative");
    if (d->part && d->part_cap < 0) return no("part_cap must not be negative");
    const int P = d->phases > 1 ? d->phases : 1;
    if (h) {
        if (!al16(d->wh)) return no("wh must be 16-B aligned");
        if (d->Cin % 8 != 0) return no("the f16 path needs Cin % 8 == 0");
        if (d->x_ts != 1) return no("the f16 path needs x_ts == 1");
        if (!d->wscale || !d->ovf) return no("the f16 path needs wscale and ovf");
        if (P > 1 && (d->wh_phase_stride < (int64_t)d->Cout * K * d->Cin || d->wh_phase_stride % 8 != 0))
            return no("wh_phase_stride below one phase's weights, or not a multiple of 8");
        if ((int64_t)(P - 1) * d->wh_phase_stride + (int64_t)d->Cout * K * d->Cin > d->n_w) return no("wh smaller than the phases' weights");
    } else {
        if (!d->w) return no("null w");
        if (d->in_scale) return no("in_scale is read by the f16 path only");
        if (P > 1 && d->w_phase_stride < (int64_t)d->Cout * K * d->Cin) return no("w_phase_stride below one phase's weights");
        if ((int64_t)(P - 1) * d->w_phase_stride + (int64_t)d->Cout * K * d->Cin > d->n_w) return no("w smaller than the phases' weights");
    }
    const int m = d->mode;
    const bool need_res = m == CV_RESID || m == CV_SUB || m == CV_ACC_FIRST || m == CV_ACC_ADD || m == CV_ACC_MEAN ||
                          m == CV_RESID_VEC || m == CV_SPLIT_RESID;
    const bool need_vec = m == CV_VEC || m == CV_RESID_VEC;
    const bool need_acc = m == CV_ACC_FIRST || m == CV_ACC_ADD || m == CV_ACC_MEAN;
    const bool need_out = !(m == CV_ACC_FIRST || m == CV_ACC_ADD);
    if (d->deferred) {
        if (d->seg) return no("seg with deferred: the slabs' consumer applies it, the conv does not read it");
        if (P > 1 || d->o_tstride != 1 || d->o_toff != 0 || d->o_len != d->n_t)
            return no("deferred needs one phase, o_tstride 1, o_toff 0 and o_len == n_t");
    }
    if (need_out && !d->out) return no("null out");
    if (need_res && (!d->res || d->r_cs < 1 || d->r_ts < 1)) return no("the mode reads res (with positive strides)");
    if (need_vec && !d->vec) return no("the mode reads vec");
    if (need_acc && !d->acc) return no("the mode reads or writes acc");
    if (m == CV_ACC_MEAN && !(d->div != 0.f)) return no("div == 0 for CV_ACC_MEAN");
    if (m == CV_SPLIT_RESID) {
        if (!d->out2 || !d->res2) return no("CV_SPLIT_RESID needs out2 and res2");
        if (d->split < 0 || d->split > d->Cout) return no("split outside 0 .. Cout");
    }
    if (d->seg && d->n_seg < d->o_len) return no("seg shorter than o_len");
    if (d->seg && need_vec && d->vec_sstride < 0) return no("vec_sstride must not be negative");

    // extents: the last element each buffer is indexed at
    if ((int64_t)(d->Cin - 1) * d->x_cs + (int64_t)(d->Tin - 1) * d->x_ts >= d->n_x) return no("x smaller than Cin x Tin at its strides");
    int64_t tp_max = (int64_t)(d->n_t - 1) * d->o_tstride + d->o_toff + (P - 1);
    if (tp_max > d->o_len - 1) tp_max = d->o_len - 1;
    if (tp_max >= 0) {
        const int rows_out = m == CV_SPLIT_RESID ? d->split : d->Cout;
        const int rows_out2 = m == CV_SPLIT_RESID ? d->Cout - d->split : 0;
        const int64_t last = tp_max * d->o_ts;
        if (need_out && rows_out > 0 && (int64_t)(rows_out - 1) * d->o_cs + last >= d->n_out) return no("out smaller than its rows x columns");
        if (rows_out2 > 0 && (int64_t)(rows_out2 - 1) * d->o_cs + last >= d->n_out2) return no("out2 / res2 smaller than their rows x columns");
        if (need_acc && (int64_t)(d->Cout - 1) * d->o_cs + last >= d->n_acc) return no("acc smaller than Cout rows x columns");
        const int rows_res = m == CV_SPLIT_RESID ? d->split : d->Cout;
        if (need_res && rows_res > 0 && (int64_t)(rows_res - 1) * d->r_cs + tp_max * d->r_ts >= d->n_res)
            return no("res smaller than its rows x columns");
    }

    a = ConvArgs{};
    a.x = d->x; a.x_cs = d->x_cs; a.x_ts = d->x_ts; a.Cin = d->Cin; a.Tin = d->Tin;
    a.w = d->w; a.Cout = d->Cout; a.K = K; a.dil = d->dil; a.pad = d->pad;
    a.bias = d->bias;
    a.out = d->out; a.o_cs = d->o_cs; a.o_ts = d->o_ts; a.n_t = d->n_t; a.o_tstride = d->o_tstride;
    a.o_toff = d->o_toff; a.o_len = d->o_len;
    a.in_act = d->in_act; a.in_slope = d->in_slope;
    a.mode = m;
    a.res = d->res; a.r_cs = d->r_cs; a.r_ts = d->r_ts;
    a.vec = d->vec; a.acc = d->acc; a.div = d->div;
    a.split = d->split; a.out2 = d->out2; a.res2 = d->res2;
    a.phases = d->phases; a.w_phase_stride = d->w_phase_stride;
    a.part = d->part; a.part_cap = d->part_cap;
    a.wh = reinterpret_cast<const __half*>(d->wh); a.wscale = d->wscale; a.ovf = d->ovf;
    a.wh_phase_stride = d->wh_phase_stride; a.in_scale = d->in_scale;
    a.seg = d->seg; a.vec_sstride = d->vec_sstride;
    a.tile_force = d->tile_force; a.ws = d->ws;

    f = conv_form(a);
    if (f.path == CP_NONE) return no("not covered");
    if (h && f.path != CP_H && f.path != CP_WS)
        return no("not covered by the f16 path (a polyphase conv needs o_tstride == phases and dil 1, a plain one o_tstride 1)");
    if (f.path == CP_F32_SPLITK && (int64_t)f.nsplit * d->Cout * d->n_t > d->part_cap) return no("part smaller than the slabs");
    if (d->deferred && (f.path == CP_F32 || f.path == CP_F32_SPLITK) && !d->part) return no("deferred needs part");
    return 0;
}

}  // namespace

extern "C" int gsv_debug_conv(const gsv_conv_desc* d, void* stream, int32_t form[4]) {
    if (!form) return bad("debug conv", "null form");
    form[0] = form[1] = form[2] = form[3] = -1;
    ConvArgs a;
    ConvForm f;
    if (int e = conv_args(d, a, f)) return e;
    const bool h = f.path == CP_H || f.path == CP_WS;
    form[0] = f.path;
    form[1] = h ? f.chunk : f.nsplit;
    form[2] = h ? f.tile : f.v4;
    form[3] = d->deferred && f.path == CP_F32_SPLITK ? f.nsplit : 0;
    if (d->dry) return 0;
    (void)hipGetLastError();
    if (d->deferred) {
        const int left = conv1d_deferred(a, (hipStream_t)stream);
        if (left != form[3]) return set_error(GSV_E_HIP, "debug conv: conv1d_deferred left another slab count than conv_form states");
    } else {
        conv1d(a, (hipStream_t)stream);
    }
    return launched("debug conv launch");
}

extern "C" int gsv_debug_mrf_pair(const gsv_mrf_desc* d, void* stream) {
    auto no = [](const std::string& m) { return bad("debug mrf_pair", m); };
    if (!d) return no("null description");
    if (d->T <= 0 || d->C <= 0) return no("T and C must be positive");
    MrfPairArgs a{};
    a.r = d->r; a.T = d->T; a.C = d->C; a.K = d->K; a.dil = d->dil;
    a.w1 = reinterpret_cast<const __half*>(d->w1); a.s1 = d->s1; a.b1 = d->b1;
    a.w2 = reinterpret_cast<const __half*>(d->w2); a.s2 = d->s2;
    a.ovf = d->ovf;
    ConvArgs& e = a.e;
    e.Cout = d->Cout; e.n_t = d->n_t; e.o_len = d->o_len; e.o_tstride = d->o_tstride; e.o_toff = d->o_toff;
    e.o_cs = d->o_cs; e.o_ts = d->o_ts; e.r_cs = d->r_cs; e.r_ts = d->r_ts;
    e.bias = d->bias2; e.res = d->r; e.mode = d->mode; e.out = d->out; e.acc = d->acc; e.div = d->div; e.seg = d->seg;
    e.phases = 1;
    if (!d->r) return no("null r");
    if (const char* why = mrf_pair_why(a)) return no(std::string("not covered: ") + why);
    const int m = d->mode;
    const bool to_acc = m == CV_ACC_FIRST || m == CV_ACC_ADD;
    if (!to_acc && !d->out) return no("null out");
    if (m != CV_RESID && !d->acc) return no("the mode reads or writes acc");
    if (m == CV_ACC_MEAN && !(d->div != 0.f)) return no("div == 0 for CV_ACC_MEAN");
    if (!al16(d->w1) || !al16(d->w2)) return no("w1 and w2 must be 16-B aligned");
    if (d->out == d->r || d->acc == d->r) return no("the output must not alias r (neighbouring blocks read r's halo)");
    const int64_t n = (int64_t)d->C * d->T;
    if (d->n_r < n) return no("r smaller than C x T");
    if (!to_acc && d->n_out < n) return no("out smaller than C x T");
    if (m != CV_RESID && d->n_acc < n) return no("acc smaller than C x T");
    if (d->seg && d->n_seg < d->T) return no("seg shorter than T");
    (void)hipGetLastError();
    if (!mrf_pair(a, (hipStream_t)stream)) return no("not covered");
    return launched("debug mrf_pair launch");
}

extern "C" int gsv_debug_mha(const gsv_mha_desc* d, void* stream) {
    auto no = [](const std::string& m) { return bad("debug mha", m); };
    if (!d) return no("null description");
    if (d->nq < 1 || d->heads < 1 || d->dk < 1) return no("nq, heads and dk must be positive");
    if (d->dk > 128) return no("dk > 128");
    if (!d->q || !d->k || !d->v || !d->out) return no("null q / k / v / out");
    if (d->q_ts < 0 || d->q_cs < 0 || d->k_ts < 0 || d->k_cs < 0 || d->v_ts < 0 || d->v_cs < 0 || d->o_ts < 0 || d->o_cs < 0)
        return no("strides must not be negative");
    if (!(d->scale != 0.f)) return no("scale must not be 0");
    const bool rel = d->ek || d->ev;
    if (rel && (d->window < 0 || d->window > 8)) return no("window > 8");
    if ((d->row_seg != nullptr) != (d->row_seg_host != nullptr)) return no("row_seg goes with its host copy");
    int64_t key_hi = 0;   // one past the last key row read
    if (d->row_seg) {
        for (int i = 0; i < d->nq; ++i) {
            const int64_t s0 = d->row_seg_host[2 * i], cnt = d->row_seg_host[2 * i + 1];
            if (cnt < 1 || cnt > MHA_MAXK_HOST) return no("a row's key count outside 1 .. 2048");
            if (s0 < 0) return no("a row_seg range leaves the key buffer");
            if (rel && (i < s0 || i >= s0 + cnt)) return no("rel-pos terms: a packed row must lie in its own key range");
            if (s0 + cnt > key_hi) key_hi = s0 + cnt;
        }
    } else {
        if (d->nk < 1 || d->nk > MHA_MAXK_HOST) return no("a row's key count outside 1 .. 2048");
        if (rel && d->nq != d->nk) return no("rel-pos terms need nq == nk (self-attention) unless row_seg is given");
        key_hi = d->nk;
    }
    const int64_t ch = (int64_t)d->heads * d->dk - 1;
    if ((int64_t)(d->nq - 1) * d->q_ts + ch * d->q_cs >= d->n_q) return no("q smaller than nq rows x heads dk channels");
    if ((int64_t)(d->nq - 1) * d->o_ts + ch * d->o_cs >= d->n_out) return no("out smaller than nq rows x heads dk channels");
    if ((key_hi - 1) * d->k_ts + ch * d->k_cs >= d->n_k) return no("a row_seg range leaves the key buffer (k)");
    if ((key_hi - 1) * d->v_ts + ch * d->v_cs >= d->n_v) return no("a row_seg range leaves the key buffer (v)");
    MhaArgs a{};
    a.q = d->q; a.q_ts = d->q_ts; a.q_cs = d->q_cs;
    a.k = d->k; a.k_ts = d->k_ts; a.k_cs = d->k_cs;
    a.v = d->v; a.v_ts = d->v_ts; a.v_cs = d->v_cs;
    a.out = d->out; a.o_ts = d->o_ts; a.o_cs = d->o_cs;
    a.nq = d->nq; a.nk = d->nk; a.heads = d->heads; a.dk = d->dk;
    a.postdiv = d->postdiv; a.scale = d->scale;
    a.ek = d->ek; a.ev = d->ev; a.window = d->window;
    a.row_seg = d->row_seg;
    (void)hipGetLastError();
    mha(a, (hipStream_t)stream);
    return launched("debug mha launch");
}

extern "C" int gsv_debug_vits_rows(const gsv_vits_rows_desc* d, void* stream) {
    auto no = [](const std::string& m) { return bad("debug vits rows", m); };
    if (!d) return no("null description");
    if (d->op < 0 || d->op > 5) return no("op: 0 .. 5");
    if (!d->out) return no("null out");
    hipStream_t s = (hipStream_t)stream;
    float* out = reinterpret_cast<float*>(d->out);
    if (d->op <= 3) {
        if (d->C < 1 || d->T < 0) return no("C must be positive and T not negative");
        if (!d->x) return no("null x");
    }
    switch (d->op) {
        case 0:
        case 1:
            if (!d->g || !d->b) return no("LayerNorm needs g and b");
            if (d->C > 256) return no("ln_channels covers C <= 256");
            if (d->op == 0 && d->seg && d->C % 16 != 0) return no("seg needs the narrow form, C % 16 == 0");
            if (d->op == 1 && d->C % 16 != 0) return no("ln_channels_slabs needs C % 16 == 0");
            if (d->op == 1 && (d->nsplit < 2 || !d->y)) return no("ln_channels_slabs needs nsplit >= 2 slabs in y");
            break;
        case 2: break;
        case 3:
            if (d->nsplit < 1) return no("wn_gate_slabs needs nsplit >= 1");
            if (!d->vec) return no("wn_gate_slabs reads vec");
            if (d->seg && d->vec_sstride < 0) return no("vec_sstride must not be negative");
            break;
        case 4:
            if (d->n < 0 || !d->x || !d->y || !d->z) return no("mean3 needs x, y, z and n >= 0");
            if (!(d->div != 0.f)) return no("div == 0");
            break;
        case 5:
            if (d->n < 0 || !d->off || !d->len) return no("seg_fill needs off, len and n >= 0");
            if (d->nseg < 1 || d->f < 1) return no("seg_fill needs nseg >= 1 and f >= 1");
            break;
    }
    if (d->op <= 3 ? d->T == 0 : d->n == 0) return 0;
    (void)hipGetLastError();
    switch (d->op) {
        case 0: ln_channels(d->x, d->y, out, d->C, d->T, d->g, d->b, s, d->seg); break;
        case 1: ln_channels_slabs(d->x, d->y, d->nsplit, d->bias, out, d->C, d->T, d->g, d->b, s, d->seg); break;
        case 2: wn_gate(d->x, out, d->C, d->T, s); break;
        case 3: wn_gate_slabs(d->x, d->nsplit, d->bias, d->vec, d->vec_sstride, d->seg, out, d->C, d->T, s); break;
        case 4: mean3(d->x, d->y, d->z, out, d->n, d->div, s); break;
        case 5: seg_fill(reinterpret_cast<int*>(d->out), d->n, d->off, d->len, d->nseg, d->f, s); break;
    }
    return launched("debug vits rows launch");
}
