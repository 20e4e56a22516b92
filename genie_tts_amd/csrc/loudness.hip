// The loudness stage: ITU-R BS.1770-4 gated loudness, sample peak and the gain to a target under
// a peak ceiling (include/genie_engine.h, gsv_loudness / gsv_audio_loudness).  The reference
// and GPT-SoVITS only clip; a server that keeps several voices plays them several dB apart.
//
// The K-weighting filter is a fourth-order recurrence over up to 2.6 M samples.  It is run in
// parallel and exactly: a hop (3200 samples, 100 ms) is one wave, a lane filters LD_SUB = 50
// samples.  Pass 1 runs every sub-chunk from zero state (float32) and combines the lanes' final
// states with a wave scan, x_in(l + d) += M^(50 d) x_in(l), in double: what a hop leaves behind
// given zero state at its start.  A chain over the hops, S(j + 1) = M^3200 S(j) + Z(j), gives
// every hop's true incoming state.  Pass 2 repeats the scan seeded with S(j), re-runs each
// sub-chunk from its true incoming state and sums the squares.  The impulse response is never
// truncated, and every sum has one order whatever the grid: no atomics.
#include "loudness.h"

#include <cmath>

#include "engine_internal.h"

using namespace gsv;

namespace {

constexpr int LD_LSTRIDE = LD_SUB + 1;   // a lane's samples in LDS: an odd stride, no bank conflict

struct KwState {
    float s1, s2, t1, t2;
};

// One sample through the shelf and the high-pass (transposed direct form II).
__device__ __forceinline__ float kw_step(const LoudFilter& F, float u, KwState& q) {
    const float y1 = fmaf(F.b0, u, q.s1);
    q.s1 = fmaf(-F.a1, y1, fmaf(F.b1, u, q.s2));
    q.s2 = fmaf(-F.a2, y1, F.b2 * u);
    const float y = fmaf(F.c0, y1, q.t1);
    q.t1 = fmaf(-F.d1, y, fmaf(F.c1, y1, q.t2));
    q.t2 = fmaf(-F.d2, y, F.c2 * y1);
    return y;
}

__device__ __forceinline__ void mat_acc(const double* P, const double* t, double* v) {   // v += P t
#pragma unroll
    for (int r = 0; r < 4; ++r)
        v[r] += P[4 * r] * t[0] + P[4 * r + 1] * t[1] + P[4 * r + 2] * t[2] + P[4 * r + 3] * t[3];
}

// Stage the wave's hop in LDS (zeros past n), take the lane's samples into x, run them from zero
// state.  v: the lane's final state.  Every wave of the block calls it (one barrier inside).
__device__ __forceinline__ void hop_zero_run(const LoudFilter& F, const float* __restrict__ audio, int n, int hop,
                                             float* xs, float (&x)[LD_SUB], double (&v)[4]) {
    const int lane = threadIdx.x & 63;
    const long long base = (long long)hop * LD_HOP;
    for (int i = lane; i < LD_HOP; i += 64) {
        const long long g = base + i;
        xs[i + i / LD_SUB] = g < n ? audio[g] : 0.f;
    }
    __syncthreads();
    KwState q{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < LD_SUB; ++k) {
        x[k] = xs[lane * LD_LSTRIDE + k];
        (void)kw_step(F, x[k], q);
    }
    v[0] = q.s1; v[1] = q.s2; v[2] = q.t1; v[3] = q.t2;
}

// Inclusive scan over the wave: v(l) = sum over k <= l of M^(50 (l - k)) v(k), ascending steps.
__device__ __forceinline__ void hop_scan(const LoudFilter& F, double (&v)[4]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double t[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = __shfl_up(v[r], 1u << k, 64);
        if (lane >= (1 << k)) mat_acc(F.sub[k], t, v);
    }
}

// Pass 1.  grid (ceil(max_hops / LD_WAVES), items): Z(hop), the state a hop leaves from zero state.
__global__ __launch_bounds__(64 * LD_WAVES) void k_loud_states(LoudFilter F, LoudWorkspace W,
                                                              const LoudItem* __restrict__ items, int slot0) {
    __shared__ float xs[LD_WAVES][64 * LD_LSTRIDE];
    const LoudItem it = items[blockIdx.y];
    const int nh = it.n > 0 ? loudness_hops(it.n) : 0;
    if ((int)blockIdx.x * LD_WAVES >= nh) return;   // (the whole block)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, hop = blockIdx.x * LD_WAVES + wave;
    float x[LD_SUB];
    double v[4];
    hop_zero_run(F, it.audio, it.n, hop, xs[wave], x, v);
    hop_scan(F, v);
    if (lane == 63 && hop < nh) {
        double* z = W.state + ((size_t)(slot0 + blockIdx.y) * LD_MAX_HOPS + hop) * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = v[r];
    }
}

// The chain across hops, one wave per item: Z(j) is replaced by S(j), the state entering hop j.
// 64 hops are loaded at once, one per lane; every lane then walks them in order.
__global__ __launch_bounds__(64) void k_loud_chain(LoudFilter F, LoudWorkspace W, const LoudItem* __restrict__ items,
                                                   int slot0) {
    const LoudItem it = items[blockIdx.x];
    const int nh = it.n > 0 ? loudness_hops(it.n) : 0, lane = threadIdx.x;
    double* Z = W.state + (size_t)(slot0 + blockIdx.x) * LD_MAX_HOPS * 4;
    double s[4] = {0, 0, 0, 0};
    for (int j0 = 0; j0 < nh; j0 += 64) {
        const int j = j0 + lane;
        double z[4] = {0, 0, 0, 0}, mine[4] = {0, 0, 0, 0};
        if (j < nh)
            for (int r = 0; r < 4; ++r) z[r] = Z[(size_t)j * 4 + r];
        const int m = min(64, nh - j0);
        for (int k = 0; k < m; ++k) {
            if (lane == k)
                for (int r = 0; r < 4; ++r) mine[r] = s[r];
            double zk[4], t[4] = {0, 0, 0, 0};
            for (int r = 0; r < 4; ++r) zk[r] = __shfl(z[r], k, 64);
            mat_acc(F.hop, s, t);
            for (int r = 0; r < 4; ++r) s[r] = t[r] + zk[r];
        }
        if (j < nh)
            for (int r = 0; r < 4; ++r) Z[(size_t)j * 4 + r] = mine[r];
    }
}

// Pass 2.  Same grid: the hop's energy (squares of the filtered samples below n) and peak.
__global__ __launch_bounds__(64 * LD_WAVES) void k_loud_energy(LoudFilter F, LoudWorkspace W,
                                                              const LoudItem* __restrict__ items, int slot0) {
    __shared__ float xs[LD_WAVES][64 * LD_LSTRIDE];
    const LoudItem it = items[blockIdx.y];
    const int nh = it.n > 0 ? loudness_hops(it.n) : 0;
    if ((int)blockIdx.x * LD_WAVES >= nh) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, hop = blockIdx.x * LD_WAVES + wave;
    float x[LD_SUB];
    double v[4], S[4] = {0, 0, 0, 0};
    hop_zero_run(F, it.audio, it.n, hop, xs[wave], x, v);
    const size_t at = (size_t)(slot0 + blockIdx.y) * LD_MAX_HOPS + hop;
    if (hop < nh)
        for (int r = 0; r < 4; ++r) S[r] = W.state[at * 4 + r];
    if (lane == 0) mat_acc(F.sub[0], S, v);   // lane 0 ran from zero state: add what S becomes over its samples
    hop_scan(F, v);
    KwState q;
    {
        const double a = __shfl_up(v[0], 1, 64), b = __shfl_up(v[1], 1, 64), c = __shfl_up(v[2], 1, 64),
                     d = __shfl_up(v[3], 1, 64);
        q = lane == 0 ? KwState{(float)S[0], (float)S[1], (float)S[2], (float)S[3]}
                      : KwState{(float)a, (float)b, (float)c, (float)d};
    }
    const long long g0 = (long long)hop * LD_HOP + lane * LD_SUB;
    float e = 0.f, pk = 0.f;
#pragma unroll
    for (int k = 0; k < LD_SUB; ++k) {
        const float y = kw_step(F, x[k], q);
        if (g0 + k < it.n) e = fmaf(y, y, e);
        pk = fmaxf(pk, fabsf(x[k]));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        e += __shfl_xor(e, d, 64);
        pk = fmaxf(pk, __shfl_xor(pk, d, 64));
    }
    if (lane == 0 && hop < nh) {
        W.energy[at] = e;
        W.peak[at] = pk;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double lufs(double z) { return -0.691 + 10.0 * log10(z); }

// The gate and the gain, one wave per item.
__global__ __launch_bounds__(64) void k_loud_gate(LoudWorkspace W, const LoudItem* __restrict__ items, int slot0) {
    const LoudItem it = items[blockIdx.x];
    if (it.n < 0) return;
    const int lane = threadIdx.x, n = it.n, nh = loudness_hops(n);
    const size_t slot = slot0 + blockIdx.x;
    const float* e = W.energy + slot * LD_MAX_HOPS;
    const float* p = W.peak + slot * LD_MAX_HOPS;
    float pk = 0.f;
    for (int j = lane; j < nh; j += 64) pk = fmaxf(pk, p[j]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d, 64));
    double L = -INFINITY;
    int kept = 0;
    if (n > 0 && n < LD_BLOCK) {   // one ungated block over all n samples
        const double z = wave_sum(lane < nh ? (double)e[lane] : 0.0) / n;
        L = lufs(z);
        kept = L > -70.0;
    } else if (n >= LD_BLOCK) {
        const int nb = n / LD_HOP - 3;
        double s = 0, c = 0;
        for (int j = lane; j < nb; j += 64) {
            const double z = ((double)e[j] + (double)e[j + 1] + (double)e[j + 2] + (double)e[j + 3]) / LD_BLOCK;
            if (lufs(z) > -70.0) { s += z; c += 1; }
        }
        s = wave_sum(s);
        c = wave_sum(c);
        if (c > 0) {
            const double gamma = lufs(s / c) - 10.0;
            s = 0; c = 0;
            for (int j = lane; j < nb; j += 64) {
                const double z = ((double)e[j] + (double)e[j + 1] + (double)e[j + 2] + (double)e[j + 3]) / LD_BLOCK;
                const double l = lufs(z);
                if (l > -70.0 && l > gamma) { s += z; c += 1; }
            }
            s = wave_sum(s);
            c = wave_sum(c);
            if (c > 0) L = lufs(s / c);
            kept = (int)c;
        }
    }
    if (lane != 0) return;
    const float Lf = (float)L;
    float gain = 1.f;
    if (kept > 0 && it.target != 0.f) {
        double g = pow(10.0, ((double)it.target - (double)Lf) / 20.0);
        if (pk > 0.f) g = fmin(g, (double)it.ceiling / (double)pk);
        gain = (float)g;
    }
    float* own = W.stats + slot * LD_STATS;
    own[0] = Lf; own[1] = pk; own[2] = gain; own[3] = (float)kept;
    if (it.stats) {
        it.stats[0] = Lf; it.stats[1] = pk; it.stats[2] = gain; it.stats[3] = (float)kept;
    }
}

void mat_mul(const double* a, const double* b, double* c) {   // c = a b (c apart from a and b)
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            c[4 * i + j] = s;
        }
}

void mat_pow(const double* m, int p, double* out) {   // out = m^p by squaring
    double r[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, b[16], t[16];
    std::copy(m, m + 16, b);
    for (; p > 0; p >>= 1) {
        if (p & 1) {
            mat_mul(r, b, t);
            std::copy(t, t + 16, r);
        }
        mat_mul(b, b, t);
        std::copy(t, t + 16, b);
    }
    std::copy(r, r + 16, out);
}

}  // namespace

void gsv::loudness_coeffs(int rate, double out[10]) {
    const double pi = 3.14159265358979323846;
    {   // the high-frequency shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        out[0] = (Vh + Vb * K / Q + K * K) / a0;
        out[1] = 2.0 * (K * K - Vh) / a0;
        out[2] = (Vh - Vb * K / Q + K * K) / a0;
        out[3] = 2.0 * (K * K - 1.0) / a0;
        out[4] = (1.0 - K / Q + K * K) / a0;
    }
    {   // the high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / rate), a0 = 1.0 + K / Q + K * K;
        out[5] = 1.0; out[6] = -2.0; out[7] = 1.0;
        out[8] = 2.0 * (K * K - 1.0) / a0;
        out[9] = (1.0 - K / Q + K * K) / a0;
    }
}

void gsv::loudness_filter(LoudFilter* f) {
    double c[10];
    loudness_coeffs(LD_RATE, c);
    f->b0 = (float)c[0]; f->b1 = (float)c[1]; f->b2 = (float)c[2]; f->a1 = (float)c[3]; f->a2 = (float)c[4];
    f->c0 = (float)c[5]; f->c1 = (float)c[6]; f->c2 = (float)c[7]; f->d1 = (float)c[8]; f->d2 = (float)c[9];
    // kw_step with u = 0, on the coefficients as rounded: the state (s1, s2, t1, t2) after one sample
    const double a1 = f->a1, a2 = f->a2, c0 = f->c0, c1 = f->c1, c2 = f->c2, d1 = f->d1, d2 = f->d2;
    const double M[16] = {-a1, 1, 0, 0,
                          -a2, 0, 0, 0,
                          c1 - d1 * c0, 0, -d1, 1,
                          c2 - d2 * c0, 0, -d2, 0};
    for (int k = 0; k < 6; ++k) mat_pow(M, LD_SUB << k, f->sub[k]);
    mat_pow(M, LD_HOP, f->hop);
}

void gsv::loudness_launch(const LoudFilter& f, const LoudWorkspace& w, const LoudItem* items, int slot0, int n,
                          int max_hops, hipStream_t s) {
    if (n <= 0) return;
    if (max_hops > 0) {
        const dim3 grid((max_hops + LD_WAVES - 1) / LD_WAVES, n);
        hipLaunchKernelGGL(k_loud_states, grid, dim3(64 * LD_WAVES), 0, s, f, w, items, slot0);
        hipLaunchKernelGGL(k_loud_chain, dim3(n), dim3(64), 0, s, f, w, items, slot0);
        hipLaunchKernelGGL(k_loud_energy, grid, dim3(64 * LD_WAVES), 0, s, f, w, items, slot0);
    }
    hipLaunchKernelGGL(k_loud_gate, dim3(n), dim3(64), 0, s, w, items, slot0);
}

// ---------------------------------------------------------------- engine side
// The workspace (about 33 KB per item slot) and the item table are made at engine creation,
// like the output stage's tables: the stage allocates nothing at first use.
int gsv_engine::loudness_init() {
    loudness_filter(&lo_filter);
    const size_t hops = (size_t)AO_SLOTS * LD_MAX_HOPS;
    lo_ws.state = (double*)dalloc(hops * 4 * sizeof(double));
    lo_ws.energy = (float*)dalloc(hops * sizeof(float));
    lo_ws.peak = (float*)dalloc(hops * sizeof(float));
    lo_ws.stats = (float*)dalloc((size_t)AO_SLOTS * LD_STATS * sizeof(float));
    lo_tab = (LoudItem*)dalloc(sizeof(LoudItem) * AO_SLOTS);
    if (!lo_ws.state || !lo_ws.energy || !lo_ws.peak || !lo_ws.stats || !lo_tab ||
        hipHostMalloc((void**)&lo_pin, sizeof(LoudItem) * AO_SLOTS, hipHostMallocDefault) != hipSuccess)
        return set_error(GSV_E_HIP, "loudness stage workspace");
    for (hipEvent_t& e : lo_ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
            return set_error(GSV_E_HIP, "loudness stage events");
    return 0;
}

int gsv::check_loudness(const gsv_loudness& l) {
    if (l.target == 0.f) return 0;
    if (!(l.target >= -50.f && l.target <= -5.f)) return set_error(GSV_E_ARG, "loudness target: -50 .. -5 LUFS (0: off)");
    if (!(l.peak >= 0.f && l.peak <= 1.f)) return set_error(GSV_E_ARG, "loudness peak ceiling: (0, 1] (0: -1 dBFS)");
    return 0;
}

// Measure items[0..m) into the workspace slots region .. region + m on stream s.  The region's
// part of the item table is refilled only after the launch that last read it has finished.
int gsv_engine::loudness_measure(const LoudItem* items, int m, int region, hipStream_t s) {
    if (!lo_tab) return set_error(GSV_E_STATE, "loudness stage not initialised");
    if (hipEventSynchronize(lo_ev[region]) != hipSuccess) return set_error(GSV_E_HIP, "loudness stage wait");
    int max_hops = 0;
    for (int j = 0; j < m; ++j) {
        lo_pin[region + j] = items[j];
        if (items[j].n > LD_MAX_N) return set_error(GSV_E_ARG, "loudness: more than 640 * 4096 samples");
        if (items[j].n > 0) max_hops = std::max(max_hops, loudness_hops(items[j].n));
    }
    hipMemcpyAsync(lo_tab + region, lo_pin + region, sizeof(LoudItem) * m, hipMemcpyHostToDevice, s);
    loudness_launch(lo_filter, lo_ws, lo_tab + region, region, m, max_hops, s);
    hipEventRecord(lo_ev[region], s);
    return 0;
}

extern "C" int gsv_loudness_coeffs(int32_t rate, double* out) {
    if (rate <= 0 || !out) return set_error(GSV_E_ARG, "bad args");
    loudness_coeffs(rate, out);
    return 0;
}

extern "C" int gsv_audio_loudness(gsv_engine* eng, const float* audio_32k, int32_t n, float* stats, void* stream) {
    if (!eng) return set_error(GSV_E_ARG, "null engine");
    if (n < 0 || n > LD_MAX_N || (n > 0 && !audio_32k) || !stats) return set_error(GSV_E_ARG, "bad args");
    hipSetDevice(eng->device);
    StreamScope sc(eng, stream);
    (void)hipGetLastError();
    const LoudItem it{audio_32k, stats, n, 0.f, 1.f, 0};
    if (int r = eng->loudness_measure(&it, 1, gsv_engine::AO_SYNC, sc.st())) return r;
    return hipGetLastError() == hipSuccess ? 0 : set_error(GSV_E_HIP, "loudness stage launch");
}

extern "C" int gsv_debug_loudness_hops(gsv_engine* eng, const float* audio, int32_t n, float* e, void* stream) {
    if (!eng) return set_error(GSV_E_ARG, "null engine");
    if (n < 0 || n > LD_MAX_N || (n > 0 && !audio) || (n >= LD_HOP && !e)) return set_error(GSV_E_ARG, "bad args");
    hipSetDevice(eng->device);
    StreamScope sc(eng, stream);
    (void)hipGetLastError();
    const LoudItem it{audio, nullptr, n, 0.f, 1.f, 0};
    if (int r = eng->loudness_measure(&it, 1, gsv_engine::AO_SYNC, sc.st())) return r;
    if (n >= LD_HOP)
        hipMemcpyAsync(e, eng->lo_ws.energy + (size_t)gsv_engine::AO_SYNC * LD_MAX_HOPS, (size_t)(n / LD_HOP) * 4,
                       hipMemcpyDeviceToDevice, sc.st());
    return hipGetLastError() == hipSuccess ? 0 : set_error(GSV_E_HIP, "loudness stage launch");
}
