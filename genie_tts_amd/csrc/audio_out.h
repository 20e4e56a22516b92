// Output stage (audio_out.hip): the engine's 32 kHz float32 audio -> another sample rate and / or
// signed 16-bit PCM, as defined in include/genie_engine.h (gsv_audio_convert).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace gsv {

constexpr int AO_RATES = 7;        // 8000, 16000, 22050, 24000, 32000, 44100, 48000
constexpr int AO_TILE = 256;       // outputs of one item per block (one per thread)
constexpr int AO_WIN = 4 * AO_TILE + 96;   // floats of input a tile needs at most: down / up <= 4, <= 81 taps

// The polyphase form of one rate's filter h (up * the normalised Kaiser sinc, float32):
// tab[p][i] = h[p + (q - 1 - i) * up], 0 past the end of h, so output k with
// t = k * down + half, n1 = t / up, p = t % up is the chain over i = 0 .. q-1 of
// tab[p][i] * x[n1 - (q - 1) + i]: ascending n, contiguous taps.  up == down (32000): a copy.
struct AudioRates {
    const float* tab[AO_RATES];
    int up[AO_RATES], down[AO_RATES], half[AO_RATES], q[AO_RATES];
};

struct AudioOutItem {
    const float* src;   // 32 kHz float32 [n_in]
    void* dst;          // float32 or int16 [n_out]
    int n_in, n_out;
    int rate;           // index into AudioRates
    int format;         // 0 float32, 1 int16
    const float* gain;  // device scalar of the loudness stage: y * gain before the conversion; null: none
    // The join stage's device record {begin, end, n_speech, n_out} (join.h); null: none, and the
    // fields above hold.  With it the item is src[begin, end) alone, n_speech samples, followed by
    // zeros up to the record's n_out; n_out above is then the host's upper bound.
    const int32_t* span;
    int pause_n;        // samples of silence behind the speech (in the record's n_out); 0 without span
    int pad;
};

int audio_rate_index(int out_rate);              // 0 -> 32000; -1: unsupported
long long audio_samples(int n_in, int out_rate); // ceil(n_in * up / down); -1: bad rate or n_in < 0
// The rates' parameters (tab left null) and one rate's float32 phase table [up][q] (host, double math).
void audio_rate_params(AudioRates* r);
std::vector<float> audio_phase_table(const AudioRates& r, int rate);
// One launch over the device table items[n]; max_n_out: the longest item's n_out.
void audio_out_launch(const AudioRates& r, const AudioOutItem* items, int n, int max_n_out, hipStream_t s);

}  // namespace gsv
