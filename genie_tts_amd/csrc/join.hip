// The sentence join: edge-silence trim and the pause between sentences (include/genie_engine.h,
// gsv_join).  GPT-SoVITS appends `fragment_interval` seconds of zeros to every fragment; a caller
// who wants an even rhythm otherwise scans, cuts and pads every sentence on the host.
//
// The frame pass gives every 10 ms frame of an item's final audio its sum of squares in double
// (a float32 squared is exact there) and marks it active above the threshold; the span pass, one
// wave per item, finds the first and last active frame and writes the span record, from which
// the output stage converts audio[begin, end) alone and appends the pause.  Every sum has one
// order whatever the grid, and nothing is accumulated across workgroups: no atomics.
#include "join.h"

#include <climits>
#include <cmath>

#include "engine_internal.h"

using namespace gsv;

namespace {

// grid (ceil(max_frames / JN_WAVES), items): one wave per frame.  Lane l takes samples l, l + 64, ..
// of the frame (five coalesced loads of the wave), sums their squares in ascending order and the
// wave reduces by a butterfly: one order for a frame wherever it runs.
__global__ __launch_bounds__(64 * JN_WAVES) void k_join_frames(JoinWorkspace W, const JoinItem* __restrict__ items,
                                                              int slot0) {
    const JoinItem it = items[blockIdx.y];
    if (it.n <= 0 || !(it.trim || it.sums)) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, f = blockIdx.x * JN_WAVES + wave;
    if (f >= join_frames(it.n) || f >= JN_MAX_FRAMES) return;   // (the whole wave; no barrier below)
    const int base = f * JN_FRAME, c = min(JN_FRAME, it.n - base);
    const float* __restrict__ x = it.audio + base;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < JN_FRAME / 64; ++k) {
        const int i = lane + 64 * k;
        const double v = i < c ? (double)x[i] : 0.0;
        s += v * v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane != 0) return;
    W.active[(size_t)(slot0 + blockIdx.y) * JN_MAX_FRAMES + f] = s > it.thresh * (double)c;
    if (it.sums) it.sums[f] = s;
}

// One wave per item: the first and last active frame by wave reductions, the guard, and the
// lengths at the item's output rate.
__global__ __launch_bounds__(64) void k_join_span(JoinWorkspace W, const JoinItem* __restrict__ items, int slot0) {
    const JoinItem it = items[blockIdx.x];
    if (it.n < 0) return;
    const int lane = threadIdx.x;
    const size_t slot = slot0 + blockIdx.x;
    int begin = 0, end = it.n;
    if (it.trim) {
        const int nf = min(join_frames(it.n), JN_MAX_FRAMES);
        const uint8_t* __restrict__ a = W.active + slot * JN_MAX_FRAMES;
        int first = INT_MAX, last = -1;
        for (int f = lane; f < nf; f += 64)
            if (a[f]) {
                first = min(first, f);
                last = f;   // (ascending f)
            }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            first = min(first, __shfl_xor(first, d, 64));
            last = max(last, __shfl_xor(last, d, 64));
        }
        if (last < 0) {
            begin = end = 0;
        } else {
            begin = max(0, JN_FRAME * first - JN_GUARD);
            end = min(it.n, JN_FRAME * (last + 1) + JN_GUARD);
        }
    }
    if (lane != 0) return;
    const int n_speech = (int)(((long long)(end - begin) * it.up + it.down - 1) / it.down);
    const int rec[JN_SPAN] = {begin, end, n_speech, n_speech + it.pause_n};
    int32_t* own = W.span + slot * JN_SPAN;
#pragma unroll
    for (int r = 0; r < JN_SPAN; ++r) {
        own[r] = rec[r];
        if (it.span) it.span[r] = rec[r];
    }
}

}  // namespace

void gsv::join_launch(const JoinWorkspace& w, const JoinItem* items, int slot0, int n, int max_frames, hipStream_t s) {
    if (n <= 0) return;
    if (max_frames > 0) {
        const dim3 grid((max_frames + JN_WAVES - 1) / JN_WAVES, n);
        hipLaunchKernelGGL(k_join_frames, grid, dim3(64 * JN_WAVES), 0, s, w, items, slot0);
    }
    hipLaunchKernelGGL(k_join_span, dim3(n), dim3(64), 0, s, w, items, slot0);
}

// ---------------------------------------------------------------- engine side
// The workspace (8 KB of flags and one record per item slot) and the item table are made at
// engine creation, like the loudness stage's: nothing is allocated at first use.
int gsv_engine::join_init() {
    jn_ws.active = (uint8_t*)dalloc((size_t)AO_SLOTS * JN_MAX_FRAMES);
    jn_ws.span = (int32_t*)dalloc((size_t)AO_SLOTS * JN_SPAN * sizeof(int32_t));
    jn_tab = (JoinItem*)dalloc(sizeof(JoinItem) * AO_SLOTS);
    if (!jn_ws.active || !jn_ws.span || !jn_tab ||
        hipHostMalloc((void**)&jn_pin, sizeof(JoinItem) * AO_SLOTS, hipHostMallocDefault) != hipSuccess)
        return set_error(GSV_E_HIP, "join stage workspace");
    return 0;
}

bool gsv::join_active(const gsv_join& j) { return j.trim != 0.f || j.pause != 0.f || j.span; }

int gsv::check_join(const gsv_join& j) {
    if (j.trim != 0.f && !(j.trim >= -80.f && j.trim <= -20.f)) return set_error(GSV_E_ARG, "trim: -80 .. -20 dBFS (0: off)");
    if (!(j.pause >= 0.f && j.pause <= 5.f)) return set_error(GSV_E_ARG, "pause: 0 .. 5 seconds");
    return 0;
}

int gsv::join_pause_samples(int out_rate, float pause) {
    if (audio_rate_index(out_rate) < 0 || !(pause >= 0.f && pause <= 5.f)) return -1;
    return (int)((double)(out_rate == 0 ? 32000 : out_rate) * (double)pause);
}

// items[0..m) into the workspace slots region .. region + m on stream s, in front of the output
// stage's launch over the same slots.  The region's part of the item table follows the output
// stage's event (audio_out waits for it before it calls this).
int gsv_engine::join_measure(const JoinItem* items, int m, int region, hipStream_t s) {
    if (!jn_tab) return set_error(GSV_E_STATE, "join stage not initialised");
    int max_frames = 0;
    for (int j = 0; j < m; ++j) {
        jn_pin[region + j] = items[j];
        if (items[j].n <= 0 || !(items[j].trim || items[j].sums)) continue;
        if (items[j].n > JN_MAX_N) return set_error(GSV_E_ARG, "trim: more than 640 * 4096 samples");
        max_frames = std::max(max_frames, join_frames(items[j].n));
    }
    hipMemcpyAsync(jn_tab + region, jn_pin + region, sizeof(JoinItem) * m, hipMemcpyHostToDevice, s);
    join_launch(jn_ws, jn_tab + region, region, m, max_frames, s);
    return 0;
}

extern "C" int gsv_join_pause_samples(int32_t out_rate, float pause) {
    const int n = join_pause_samples(out_rate, pause);
    return n < 0 ? GSV_E_ARG : n;
}

extern "C" int gsv_join_samples(int32_t n_in, int32_t out_rate, float pause) {
    const long long n = audio_samples(n_in, out_rate);
    const int p = join_pause_samples(out_rate, pause);
    return n < 0 || p < 0 || n + p > INT32_MAX ? GSV_E_ARG : (int)(n + p);
}

extern "C" int gsv_debug_join_frames(gsv_engine* eng, const float* audio, int32_t n, double* sums, void* stream) {
    if (!eng) return set_error(GSV_E_ARG, "null engine");
    if (n < 0 || n > JN_MAX_N || (n > 0 && (!audio || !sums))) return set_error(GSV_E_ARG, "bad args");
    hipSetDevice(eng->device);
    StreamScope sc(eng, stream);
    (void)hipGetLastError();
    hipEvent_t ev = eng->ao_ev[gsv_engine::AO_SYNC];
    if (hipEventSynchronize(ev) != hipSuccess) return set_error(GSV_E_HIP, "output stage wait");
    const JoinItem it{audio, nullptr, sums, 0.0, n, 0, 1, 1, 0, 0};
    if (int r = eng->join_measure(&it, 1, gsv_engine::AO_SYNC, sc.st())) return r;
    hipEventRecord(ev, sc.st());
    return hipGetLastError() == hipSuccess ? 0 : set_error(GSV_E_HIP, "join stage launch");
}
