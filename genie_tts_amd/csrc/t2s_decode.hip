// Fused decode-step kernels (B small, latency-bound): one T2S layer of the
// stage decoder (t2s_stage_decoder_fp32.onnx#43-114 per layer) runs as three
// launches instead of five:
//   1. QKV GEMV            prologue: reduce the previous layer's FFN2 split-K
//                          partials + residual, LayerNorm2 (k_gemv, t2s.hip)
//   2. attention + out-proj split over heads (this file)
//   3. FFN1 + FFN2 split over the hidden units; prologue reduces the
//      out-proj partials + residual, LayerNorm1 (this file)
// Partial sums are reduced in a fixed order (deterministic).
#include "common.h"
#include "kernels.h"
#include <hip/hip_ext.h>

namespace gsv {

// ---------------------------------------------------------------------------
// Attention (one head, one sequence) + out-projection partial for that head.
// ---------------------------------------------------------------------------
// Reduce-scatter of a 32-vector over the 64 lanes of a wave: afterwards lane l
// holds sum over all lanes of a[l & 31].
__device__ __forceinline__ float wave_reduce_scatter32(float (&a)[32]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
        const bool up = (lane & s) != 0;
#pragma unroll
        for (int j = 0; j < s; ++j) {
            const float send = up ? a[j] : a[j + s];
            const float keep = up ? a[j + s] : a[j];
            a[j] = keep + __shfl_xor(send, s, 64);
        }
    }
    return a[0] + __shfl_xor(a[0], 32, 64);
}

// Lane layout: 8 lanes per key row (lane & 7 = 16-byte chunk c of the 128-byte
// K/V head row), 8 keys per wave instruction, 32 keys per block pass: every
// load instruction reads 1 KB contiguous.  Each lane keeps an online softmax
// state (m, l) and the 4 output dims of its chunk.
__global__ __launch_bounds__(256) void k_attn_out(AttnOutArgs a) {
    __shared__ float os[32];
    __shared__ float redm[4];
    __shared__ float redl[4][8];
    __shared__ float reda[4][32];
    __shared__ float ored[4][512];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    GSV_STAMP(a.trace, 0);
    // Issue order = retire order (vmcnt): done/kvlen/q first, then the first 256
    // K/V rows speculatively (rows < tmax are allocated; rows >= len are masked by
    // selects, so stale contents never reach the math), then -- once len is known --
    // the rest of the first pass, then the WoT slice.
    const uint8_t dn = a.done ? a.done[b] : 0;
    const int lenv = a.kvlen[b];
    const float* K = a.k + (long)b * a.seq_stride + (long)h * a.tmax * 32;
    const float* V = a.v + (long)b * a.seq_stride + (long)h * a.tmax * 32;
    const float sc = a.scale;
    const int c = lane & 7, g = (w << 3) | (lane >> 3);     // chunk, key group (0..31)
    const float4 qv = *reinterpret_cast<const float4*>(a.q + (long)b * 512 + h * 32 + 4 * c);
    constexpr int U = 16, US = 8;                            // keys per group per pass; speculative part
    float4 kk[U], vv[U];
#pragma unroll
    for (int u = 0; u < US; ++u) {
        const int t = min(u * 32 + g, a.tmax - 1);
        kk[u] = *reinterpret_cast<const float4*>(K + (long)t * 32 + 4 * c);
        vv[u] = *reinterpret_cast<const float4*>(V + (long)t * 32 + 4 * c);
    }
    if (dn) return;
    const int len = lenv + 1;
#pragma unroll
    for (int u = US; u < U; ++u) {
        const int t = u * 32 + g;
        if (t < len) {
            kk[u] = *reinterpret_cast<const float4*>(K + (long)t * 32 + 4 * c);
            vv[u] = *reinterpret_cast<const float4*>(V + (long)t * 32 + 4 * c);
        } else {
            kk[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            vv[u] = kk[u];
        }
    }
    uint4 wo[8];
    {
        const __half* wb = a.WoT + (long)(h * 32) * 512 + 8 * lane;
#pragma unroll
        for (int i = 0; i < 8; ++i) wo[i] = *reinterpret_cast<const uint4*>(wb + (long)(w + 4 * i) * 512);
    }
    const float q0 = qv.x * sc, q1 = qv.y * sc, q2 = qv.z * sc, q3 = qv.w * sc;
    float mt = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
    // One pass = 32 groups x U keys, every row of the pass in registers before any
    // math; the per-lane softmax state is merged once per pass.
    for (int base = 0; base < len; base += 32 * U) {
        if (base > 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = base + u * 32 + g;
                if (t < len) {
                    kk[u] = *reinterpret_cast<const float4*>(K + (long)t * 32 + 4 * c);
                    vv[u] = *reinterpret_cast<const float4*>(V + (long)t * 32 + 4 * c);
                }
            }
        }
        float sv[U];
        float pm = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float x = q0 * (kk[u].x * sc);
            x += q1 * (kk[u].y * sc);
            x += q2 * (kk[u].z * sc);
            x += q3 * (kk[u].w * sc);
            // sum over the 8 lanes of the key row: quad swaps, then the half-row mirror
            x += dpp_f<0xB1, 0xF>(x);
            x += dpp_f<0x4E, 0xF>(x);
            x += dpp_f<0x141, 0xF>(x);
            const bool valid = base + u * 32 + g < len;       // uniform within the 8-lane group
            sv[u] = valid ? x : -INFINITY;
            if (!valid) vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            pm = fmaxf(pm, sv[u]);
        }
        if (pm == -INFINITY) continue;                          // this group has no key in the pass
        const float mn = fmaxf(mt, pm);
        const float f = expf(mt - mn);
        float ls = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float p = expf(sv[u] - mn);
            ls += p;
            a0 += p * vv[u].x;
            a1 += p * vv[u].y;
            a2 += p * vv[u].z;
            a3 += p * vv[u].w;
        }
        l = l * f + ls;
        o0 = o0 * f + a0;
        o1 = o1 * f + a1;
        o2 = o2 * f + a2;
        o3 = o3 * f + a3;
        mt = mn;
    }
    GSV_STAMP(a.trace, 1);
    // block max of the per-group maxima
    const float bm = wave_max(mt);
    if (lane == 0) redm[w] = bm;
    __syncthreads();
    const float m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
    const float fs = mt == -INFINITY ? 0.f : expf(mt - m);
    l *= fs; o0 *= fs; o1 *= fs; o2 *= fs; o3 *= fs;
    // sum over the 8 key groups of this wave (lanes with equal chunk c)
#pragma unroll
    for (int x = 8; x < 64; x <<= 1) {
        l += __shfl_xor(l, x, 64);
        o0 += __shfl_xor(o0, x, 64);
        o1 += __shfl_xor(o1, x, 64);
        o2 += __shfl_xor(o2, x, 64);
        o3 += __shfl_xor(o3, x, 64);
    }
    if (lane < 8) {
        reda[w][4 * lane] = o0; reda[w][4 * lane + 1] = o1;
        reda[w][4 * lane + 2] = o2; reda[w][4 * lane + 3] = o3;
        redl[w][lane] = l;
    }
    __syncthreads();
    if (tid < 32) {
        const float L = (redl[0][0] + redl[1][0]) + (redl[2][0] + redl[3][0]);
        os[tid] = ((reda[0][tid] + reda[1][tid]) + (reda[2][tid] + reda[3][tid])) / L;
    }
    __syncthreads();
    GSV_STAMP(a.trace, 2);
    float r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float wf[8];
        h8_to_f8(wo[i], wf);
        const float ov = os[w + 4 * i];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += wf[k] * ov;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) ored[w][8 * lane + k] = r[k];
    __syncthreads();
    const float r0 = (ored[0][tid] + ored[1][tid]) + (ored[2][tid] + ored[3][tid]);
    const float r1 = (ored[0][tid + 256] + ored[1][tid + 256]) + (ored[2][tid + 256] + ored[3][tid + 256]);
    if (a.acc_out) {
        long long* ac = a.acc_out + (long)b * a.acc_bstride;
        fx_add(ac + tid, r0);
        fx_add(ac + tid + 256, r1);
    } else {
        float* dst = a.part + ((long)h * a.B + b) * 512;
        dst[tid] = r0;
        dst[tid + 256] = r1;
    }
    GSV_STAMP(a.trace, 3);
}

void attn_outproj(const AttnOutArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_attn_out, dim3(16, a.B), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------
// FFN1 + FFN2 (split-K over hidden units); RPB hidden rows per block.
// ---------------------------------------------------------------------------
template <int RPB, int NB>
__global__ __launch_bounds__(256) void k_ffn(FfnArgs a) {
    __shared__ float xs[NB][512];
    __shared__ float fs[NB][RPB];
    __shared__ float red[4 * NB * 2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = blockIdx.x, B = a.B;
    GSV_STAMP(a.trace, 0);
    constexpr int RW = RPB / 4;            // FFN1 rows per wave
    // small parameters now, not after the barriers
    const float lng0 = a.ln_g[tid], lng1 = a.ln_g[tid + 256], lnb0 = a.ln_b[tid], lnb1 = a.ln_b[tid + 256];
    float b1r[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) b1r[r] = a.b1[j * RPB + w * RW + r];
    // prologue: s1 = h + (bo + sum_h attn_part[h]); LN1
    float v0[NB], v1[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b >= B) break;
        float p0 = a.bo[tid], p1 = a.bo[tid + 256];
        if (a.acc_attn) {
            const long long* ac = a.acc_attn + (long)b * a.acc_bstride;
            p0 += from_fx(ac[tid]);
            p1 += from_fx(ac[tid + 256]);
        } else {
#pragma unroll
            for (int hh = 0; hh < 16; ++hh) {
                const float* pp = a.attn_part + ((long)hh * B + b) * 512;
                p0 += pp[tid];
                p1 += pp[tid + 256];
            }
        }
        v0[b] = a.h[(long)b * 512 + tid] + p0;
        v1[b] = a.h[(long)b * 512 + tid + 256] + p1;
    }
    // Weight prefetch AFTER the prologue loads: vmcnt retires in order, so loads
    // issued after the 64 KB weight stream would wait for all of it.
    // FFN1 rows (one 16 B chunk per lane per row) and the W2T slice rows
    // j*RPB + w + 4*i (i < RPB/4), columns [8*lane, +8)
    uint4 w1r[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r)
        w1r[r] = *reinterpret_cast<const uint4*>(a.W1 + (long)(j * RPB + w * RW + r) * 512 + lane * 8);
    uint4 w2r[RPB / 4];
#pragma unroll
    for (int i = 0; i < RPB / 4; ++i)
        w2r[i] = *reinterpret_cast<const uint4*>(a.W2T + (long)(j * RPB + w + 4 * i) * 512 + 8 * lane);
    float mean[NB], den[NB];
    block_meanvar512<NB>(v0, v1, B, mean, den, red);
    GSV_STAMP(a.trace, 1);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b >= B) break;
        const float o0 = (v0[b] - mean[b]) / den[b] * lng0 + lnb0;
        const float o1 = (v1[b] - mean[b]) / den[b] * lng1 + lnb1;
        xs[b][tid] = o0;
        xs[b][tid + 256] = o1;
        if (j == 0) {
            a.h1[(long)b * 512 + tid] = o0;
            a.h1[(long)b * 512 + tid + 256] = o1;
        }
    }
    __syncthreads();
    // FFN1 rows of this slice
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        float wf[8];
        h8_to_f8(w1r[r], wf);
        const int row = j * RPB + w * RW + r;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b >= B) break;
            const float4 x0 = *reinterpret_cast<const float4*>(&xs[b][lane * 8]);
            const float4 x1 = *reinterpret_cast<const float4*>(&xs[b][lane * 8 + 4]);
            float s = 0.f;
            s += wf[0] * x0.x; s += wf[1] * x0.y; s += wf[2] * x0.z; s += wf[3] * x0.w;
            s += wf[4] * x1.x; s += wf[5] * x1.y; s += wf[6] * x1.z; s += wf[7] * x1.w;
            s = wave_sum_dpp(s);
            if (lane == 0) fs[b][w * RW + r] = fmaxf(b1r[r] + s, 0.f);
        }
    }
    __syncthreads();
    GSV_STAMP(a.trace, 2);
    // FFN2 partial: each wave sums its rows for 8 columns per lane, then LDS reduce
    __shared__ float fred[4][512];
    for (int b = 0; b < B; ++b) {
        float r8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r8[k] = 0.f;
#pragma unroll
        for (int i = 0; i < RPB / 4; ++i) {
            float wf[8];
            h8_to_f8(w2r[i], wf);
            const float fv = fs[b][w + 4 * i];
#pragma unroll
            for (int k = 0; k < 8; ++k) r8[k] += wf[k] * fv;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) fred[w][8 * lane + k] = r8[k];
        __syncthreads();
        const float r0 = (fred[0][tid] + fred[1][tid]) + (fred[2][tid] + fred[3][tid]);
        const float r1 = (fred[0][tid + 256] + fred[1][tid + 256]) + (fred[2][tid + 256] + fred[3][tid + 256]);
        if (a.acc_out) {
            long long* ac = a.acc_out + (long)b * a.acc_bstride;
            fx_add(ac + tid, r0);
            fx_add(ac + tid + 256, r1);
        } else {
            float* dst = a.part + ((long)j * B + b) * 512;
            dst[tid] = r0;
            dst[tid + 256] = r1;
        }
        __syncthreads();
    }
    GSV_STAMP(a.trace, 3);
}

// start/stop (optional): hipExtLaunchKernelGGL stamps them from the dispatch packet's
// own begin/end timestamps -- the bench's live per-launch duration of this kernel.
template <int RPB>
static void launch_ffn(const FfnArgs& a, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    const int nb = a.B <= 1 ? 1 : a.B <= 2 ? 2 : a.B <= 4 ? 4 : 8;
    const dim3 g(a.nslices), blk(256);
    switch (nb) {
        case 1: hipExtLaunchKernelGGL((k_ffn<RPB, 1>), g, blk, 0, s, start, stop, 0, a); break;
        case 2: hipExtLaunchKernelGGL((k_ffn<RPB, 2>), g, blk, 0, s, start, stop, 0, a); break;
        case 4: hipExtLaunchKernelGGL((k_ffn<RPB, 4>), g, blk, 0, s, start, stop, 0, a); break;
        default: hipExtLaunchKernelGGL((k_ffn<RPB, 8>), g, blk, 0, s, start, stop, 0, a); break;
    }
}

void ffn_fused(const FfnArgs& a, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    if (a.nslices == 64) launch_ffn<32>(a, s, start, stop);
    else launch_ffn<64>(a, s, start, stop);   // nslices == 32
}

}  // namespace gsv
