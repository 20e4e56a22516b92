// Loudness stage (loudness.hip): ITU-R BS.1770-4 gated loudness of an item's 32 kHz float32
// audio, its sample peak and the gain to a target under a peak ceiling, as defined in
// include/genie_engine.h (gsv_loudness, gsv_audio_loudness).  The gain stays on the device: the
// output stage (audio_out.hip) reads it through AudioOutItem::gain.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsv {

constexpr int LD_RATE = 32000;
constexpr int LD_HOP = 3200;             // 100 ms: one wave, 64 lanes x LD_SUB samples
constexpr int LD_SUB = 50;               // samples a lane filters sequentially
constexpr int LD_BLOCK = 4 * LD_HOP;     // 400 ms gating block = 4 hops (75 % overlap)
constexpr int LD_WAVES = 4;              // hops per workgroup
constexpr int LD_MAX_N = 640 * 4096;     // longest vocoder output
constexpr int LD_MAX_HOPS = (LD_MAX_N + LD_HOP - 1) / LD_HOP;   // 820, the partial last hop included
constexpr int LD_STATS = 4;              // loudness_lufs, peak, gain, blocks_kept

// The K-weighting filter as the engine runs it: two biquads in transposed direct form II with
// float32 coefficients, and what carries its 4-element state (s1, s2 of the shelf, t1, t2 of the
// high-pass) over a run of zero input: powers of the state-transition matrix M of those rounded
// coefficients, row-major, built on the host in double.
struct LoudFilter {
    float b0, b1, b2, a1, a2;   // shelf
    float c0, c1, c2, d1, d2;   // high-pass
    double sub[6][16];          // M^(LD_SUB * 2^k), k = 0..5: the wave scan's steps
    double hop[16];             // M^LD_HOP: the chain across hops
};

// One item of a measurement launch.  n < 0 skips the slot.
struct LoudItem {
    const float* audio;   // 32 kHz float32 [n]
    float* stats;         // the caller's device float[LD_STATS], or null
    int n;
    float target;         // LUFS; 0: measure only (gain 1)
    float ceiling;        // linear peak ceiling
    int pad;
};

// Per item slot: the hops' carried states (double[4] each), energies and peaks, and the stats.
struct LoudWorkspace {
    double* state;   // [slots][LD_MAX_HOPS][4]
    float* energy;   // [slots][LD_MAX_HOPS]
    float* peak;     // [slots][LD_MAX_HOPS]
    float* stats;    // [slots][LD_STATS]
};

// K-weighting coefficients at `rate` (double): out = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2.
void loudness_coeffs(int rate, double out[10]);
void loudness_filter(LoudFilter* f);   // at LD_RATE
__host__ __device__ inline int loudness_hops(int n) { return (n + LD_HOP - 1) / LD_HOP; }
// Measure items[0..n) (device table; item i uses workspace slot slot0 + i): four launches on s.
void loudness_launch(const LoudFilter& f, const LoudWorkspace& w, const LoudItem* items, int slot0, int n,
                     int max_hops, hipStream_t s);

}  // namespace gsv
