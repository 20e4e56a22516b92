// Sentence join (join.hip): where an item's speech begins and ends, measured on the GPU over
// 10 ms frames of its 32 kHz float32 audio, and the pause appended behind it, as defined in
// include/genie_engine.h (gsv_join).  The span stays on the device: the output stage
// (audio_out.hip) reads it through AudioOutItem::span, converts only that span and writes the
// pause's zeros.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/genie_engine.h"

namespace gsv {

constexpr int JN_FRAME = GSV_JOIN_FRAME;   // 10 ms: one wave, 64 lanes x 5 samples
constexpr int JN_GUARD = GSV_JOIN_GUARD;   // 20 ms kept on either side of the active frames
constexpr int JN_WAVES = 4;                // frames per workgroup
constexpr int JN_MAX_N = 640 * 4096;       // longest vocoder output
constexpr int JN_MAX_FRAMES = JN_MAX_N / JN_FRAME;   // 8192
constexpr int JN_SPAN = 4;                 // begin, end, n_speech, n_out

// One item of a join launch.  n < 0 skips the slot.
struct JoinItem {
    const float* audio;   // 32 kHz float32 [n]
    int32_t* span;        // the caller's device int32[JN_SPAN], or null
    double* sums;         // debug: the frames' sums of squares [frames], or null
    double thresh;        // T = 10^(trim / 10): frame f is active when its sum > T * its samples
    int n;
    int trim;             // 0: the span is [0, n)
    int up, down;         // of the item's output rate: n_speech = ceil((end - begin) * up / down)
    int pause_n;          // samples of silence behind the speech, at the output rate
    int pad;
};

// Per item slot: the frames' active flags and the span record the output stage reads.
struct JoinWorkspace {
    uint8_t* active;   // [slots][JN_MAX_FRAMES]
    int32_t* span;     // [slots][JN_SPAN]
};

__host__ __device__ inline int join_frames(int n) { return (n + JN_FRAME - 1) / JN_FRAME; }
// Items[0..n) (device table; item i uses workspace slot slot0 + i) on s: the frame pass when
// max_frames > 0 (the most frames of an item that measures), then the span pass.
void join_launch(const JoinWorkspace& w, const JoinItem* items, int slot0, int n, int max_frames, hipStream_t s);

}  // namespace gsv
