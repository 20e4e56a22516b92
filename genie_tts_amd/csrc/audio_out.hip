// The output stage: sample rate and 16-bit PCM (include/genie_engine.h, gsv_audio_convert).
// A rational polyphase resample of the 32 kHz float32 audio with scipy.signal.resample_poly's
// default filter (Kaiser 5.0 windowed sinc, 10 * max(up, down) taps a side), restated here so
// nothing depends on scipy at run time, then the optional int16 conversion.  The reference
// delivers (x * 32767).astype(int16) chunks at 32 kHz only (Core/TTSPlayer.py).
#include "audio_out.h"

#include <cmath>
#include <numeric>

#include "engine_internal.h"

using namespace gsv;

namespace {

constexpr int RATES[AO_RATES] = {8000, 16000, 22050, 24000, 32000, 44100, 48000};

double bessel_i0(double x) {   // the power series sum_k ((x / 2)^k / k!)^2
    const double y = x * x / 4;
    double term = 1, sum = 1;
    for (int k = 1; k < 200; ++k) {
        term *= y / ((double)k * k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// One block: AO_TILE consecutive outputs of item blockIdx.y.  The input window those outputs
// need is staged in LDS with the zeros outside [0, n_in) written explicitly, so an item never
// reads its neighbour in a packed buffer.  Each output is one float32 fma chain over ascending
// n whatever the tile: the same bits from every entry point.
__global__ __launch_bounds__(AO_TILE) void k_audio_out(AudioRates R, const AudioOutItem* __restrict__ items) {
    __shared__ float xs[AO_WIN];
    const AudioOutItem it = items[blockIdx.y];
    const int k0 = blockIdx.x * AO_TILE;
    // With a span record (join.hip) the item is src[begin, end) alone, n_speech outputs, and the
    // pause's zeros up to n_out; all four are read here, on the device.
    const float* __restrict__ src = it.src;
    int n_in = it.n_in, n_out = it.n_out, n_speech = it.n_out;
    if (it.span) {
        const int begin = it.span[0], end = it.span[1];
        src += begin;
        n_in = end - begin;
        n_speech = it.span[2];
        n_out = min(it.span[3], it.n_out);
    }
    if (k0 >= n_out) return;
    const int k = k0 + (int)threadIdx.x;
    const int up = R.up[it.rate], down = R.down[it.rate];
    float y = 0.f;
    if (up == down) {   // 32000: a copy (n_speech == n_in)
        if (k < n_speech) y = src[k];
    } else if (k0 < n_speech) {   // (the whole block: a tile of the pause alone stages nothing)
        const int half = R.half[it.rate], q = R.q[it.rate];
        const float* __restrict__ tab = R.tab[it.rate];
        const int k1 = min(k0 + AO_TILE, n_speech) - 1;   // the tile's last output
        const long long lo = ((long long)k0 * down + half) / up - (q - 1);
        const long long hi = ((long long)k1 * down + half) / up;
        const int win = min((int)(hi - lo + 1), AO_WIN);   // (<= AO_WIN for every supported rate)
        for (int i = threadIdx.x; i < win; i += AO_TILE) {
            const long long n = lo + i;
            xs[i] = n >= 0 && n < n_in ? src[n] : 0.f;
        }
        __syncthreads();
        if (k < n_speech) {
            const long long t = (long long)k * down + half;
            const long long n1 = t / up;
            const float* __restrict__ c = tab + (size_t)(t - n1 * up) * q;
            const float* x = xs + (int)(n1 - (q - 1) - lo);
            for (int i = 0; i < q; ++i) y = fmaf(c[i], x[i], y);
        }
    }
    if (k >= n_out) return;
    if (k >= n_speech) y = 0.f;   // the pause: +0.0f / int16 0, whatever the gain
    else if (it.gain) y = y * *it.gain;   // loudness normalisation: one rounded multiply behind the chain
    if (it.format == 0) {
        ((float*)it.dst)[k] = y;
    } else {   // (x * 32767).astype(int16) of the reference, saturated
        const float v = fminf(fmaxf(y * 32767.0f, -32768.0f), 32767.0f);
        ((int16_t*)it.dst)[k] = (int16_t)(int)v;
    }
}

}  // namespace

int gsv::audio_rate_index(int out_rate) {
    if (out_rate == 0) out_rate = 32000;
    for (int i = 0; i < AO_RATES; ++i)
        if (RATES[i] == out_rate) return i;
    return -1;
}

long long gsv::audio_samples(int n_in, int out_rate) {
    const int i = audio_rate_index(out_rate);
    if (i < 0 || n_in < 0) return -1;
    const int g = std::gcd(32000, RATES[i]);
    const long long up = RATES[i] / g, down = 32000 / g;
    return ((long long)n_in * up + down - 1) / down;
}

void gsv::audio_rate_params(AudioRates* r) {
    for (int i = 0; i < AO_RATES; ++i) {
        const int g = std::gcd(32000, RATES[i]);
        r->tab[i] = nullptr;
        r->up[i] = RATES[i] / g;
        r->down[i] = 32000 / g;
        r->half[i] = 10 * std::max(r->up[i], r->down[i]);
        r->q[i] = (2 * r->half[i] + 1 + r->up[i] - 1) / r->up[i];
    }
}

std::vector<float> gsv::audio_phase_table(const AudioRates& r, int rate) {
    const int up = r.up[rate], half = r.half[rate], q = r.q[rate], len = 2 * half + 1;
    const double m = std::max(up, r.down[rate]), pi = 3.14159265358979323846, i0b = bessel_i0(5.0);
    std::vector<double> h(len);
    double sum = 0;
    for (int i = 0; i < len; ++i) {
        const double t = (i - half) / m, u = (double)(i - half) / half;
        const double sinc = i == half ? 1.0 : std::sin(pi * t) / (pi * t);
        h[i] = (1.0 / m) * sinc * bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
        sum += h[i];
    }
    std::vector<float> tab((size_t)up * q, 0.f);
    for (int p = 0; p < up; ++p)
        for (int i = 0; i < q; ++i) {
            const int j = p + (q - 1 - i) * up;
            if (j < len) tab[(size_t)p * q + i] = (float)(h[j] / sum * up);   // rounded once to float32
        }
    return tab;
}

void gsv::audio_out_launch(const AudioRates& r, const AudioOutItem* items, int n, int max_n_out, hipStream_t s) {
    if (n <= 0 || max_n_out <= 0) return;
    const dim3 grid((max_n_out + AO_TILE - 1) / AO_TILE, n);
    hipLaunchKernelGGL(k_audio_out, grid, dim3(AO_TILE), 0, s, r, items);
}

// ---------------------------------------------------------------- engine side
// The six tables (about 22k floats) and the item table are made at engine creation: nothing
// is allocated or built at first use, so the stage stays out of stream captures.
int gsv_engine::audio_out_init() {
    audio_rate_params(&ao_rates);
    std::unique_lock<std::shared_mutex> cl(gsv::capture_mu);   // synchronous null-stream copies below
    for (int i = 0; i < AO_RATES; ++i) {
        if (ao_rates.up[i] == ao_rates.down[i]) continue;
        const std::vector<float> t = audio_phase_table(ao_rates, i);
        float* d = (float*)dalloc(t.size() * 4);
        if (!d || hipMemcpy(d, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return set_error(GSV_E_HIP, "output stage tables");
        ao_rates.tab[i] = d;
    }
    if (int r = loudness_init()) return r;
    if (int r = join_init()) return r;
    ao_tab = (AudioOutItem*)dalloc(sizeof(AudioOutItem) * AO_SLOTS);
    if (!ao_tab || hipHostMalloc((void**)&ao_pin, sizeof(AudioOutItem) * AO_SLOTS, hipHostMallocDefault) != hipSuccess)
        return set_error(GSV_E_HIP, "output stage item table");
    for (hipEvent_t& e : ao_ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
            return set_error(GSV_E_HIP, "output stage events");
    return 0;
}

int gsv_engine::audio_item(const gsv_vits_item& u, AudioOutItem* a) const {
    const int rate = audio_rate_index(u.out_rate), T = vits_frames(u.n_sem, u.speed);
    if (rate < 0 || u.out_format < 0 || u.out_format > 1 || T < 0) return GSV_E_ARG;
    const int n_in = 640 * T;
    *a = AudioOutItem{u.audio, u.out, n_in, (int)audio_samples(n_in, u.out_rate), rate, u.out_format, nullptr};
    return 0;
}

// Convert items[0..n) in one launch per AO_BATCH items on stream s.  `region` names the part of
// the item table this call site owns (AO_SYNC: the engine stream's synchronous calls, AO_ASYNC:
// the overlapped vocoder call, AO_BATCH_AT: a batch): a region is refilled only after the launch
// that last read it has finished, which it has in practice (the wait is for the previous call's
// stage, and a vocoder pass lies between two of them).  spec (null: none) lies beside items: the
// entries with a target are measured first, one pass per launch (loudness.hip), and their
// conversions read the gain from the measurement's slot on the device.  The entries with a trim,
// a pause or a span record go through the join stage the same way (join.hip): their conversions
// read the span from the slot's record, and n_out of their table entry is the host's upper bound.
// An all-zero entry is the same as none: no measurement, no launch, the table entry as it is.
int gsv_engine::audio_out(const AudioOutItem* items, const gsv_join* spec, int n, int region, hipStream_t s) {
    if (!ao_tab) return set_error(GSV_E_STATE, "output stage not initialised");
    const int base = region, cap = region == AO_BATCH_AT ? AO_BATCH : 1;   // (a region is its first slot)
    hipEvent_t ev = ao_ev[region];
    (void)hipGetLastError();
    for (int i = 0; i < n; i += cap) {
        const int m = std::min(cap, n - i);
        if (hipEventSynchronize(ev) != hipSuccess) return set_error(GSV_E_HIP, "output stage wait");
        int max_out = 0;
        std::vector<LoudItem> loud;
        std::vector<JoinItem> join;
        for (int j = 0; j < m; ++j) {
            ao_pin[base + j] = items[i + j];
            if (spec && join_active(spec[i + j])) {
                // its span goes into slot base + j's record, which this item's conversion reads on the device
                const gsv_join& l = spec[i + j];
                const AudioOutItem& a = items[i + j];
                const int pause_n = join_pause_samples(RATES[a.rate], l.pause);
                if (pause_n < 0) return set_error(GSV_E_ARG, "pause: 0 .. 5 seconds");
                join.resize(m, JoinItem{nullptr, nullptr, nullptr, 0.0, -1, 0, 1, 1, 0, 0});
                join[j] = JoinItem{a.src, l.span, nullptr, l.trim != 0.f ? std::pow(10.0, (double)l.trim / 10.0) : 0.0,
                                   a.n_in, l.trim != 0.f, ao_rates.up[a.rate], ao_rates.down[a.rate], pause_n, 0};
                ao_pin[base + j].span = jn_ws.span + (size_t)(base + j) * JN_SPAN;
                ao_pin[base + j].pause_n = pause_n;
                ao_pin[base + j].n_out += pause_n;
            }
            max_out = std::max(max_out, ao_pin[base + j].n_out);
            if (!spec || spec[i + j].target == 0.f) continue;
            // measured into slot base + j, whose gain this item's conversion reads on the device
            const gsv_join& l = spec[i + j];
            loud.resize(m, LoudItem{nullptr, nullptr, -1, 0.f, 1.f, 0});
            loud[j] = LoudItem{items[i + j].src, l.stats, items[i + j].n_in, l.target,
                               l.peak == 0.f ? 0.8912509381337456f : l.peak, 0};
            ao_pin[base + j].gain = lo_ws.stats + (size_t)(base + j) * LD_STATS + 2;
        }
        if (!loud.empty())
            if (int r = loudness_measure(loud.data(), m, base, s)) return r;
        if (!join.empty())
            if (int r = join_measure(join.data(), m, base, s)) return r;
        hipMemcpyAsync(ao_tab + base, ao_pin + base, sizeof(AudioOutItem) * m, hipMemcpyHostToDevice, s);
        audio_out_launch(ao_rates, ao_tab + base, m, max_out, s);
        hipEventRecord(ev, s);
    }
    return hipGetLastError() == hipSuccess ? 0 : set_error(GSV_E_HIP, "output stage launch");
}

// The items of a vocoder call that carry `out`, converted from their final `audio`.
int gsv_engine::audio_out_items(const gsv_vits_item* it, const gsv_join* spec, int n, int region, hipStream_t s) {
    std::vector<AudioOutItem> a;
    std::vector<gsv_join> l;
    for (int i = 0; i < n; ++i) {
        if (!it[i].out) continue;
        a.emplace_back();
        if (audio_item(it[i], &a.back())) return set_error(GSV_E_ARG, "bad output rate or format");
        if (spec) l.push_back(spec[i]);
    }
    return a.empty() ? 0 : audio_out(a.data(), spec ? l.data() : nullptr, (int)a.size(), region, s);
}

extern "C" int gsv_audio_samples(int32_t n_in, int32_t out_rate) {
    const long long n = audio_samples(n_in, out_rate);
    return n < 0 || n > INT32_MAX ? GSV_E_ARG : (int)n;
}

int gsv::check_spec(const gsv_join& spec, bool has_out, int n_in) {
    if (int r = check_loudness(gsv_loudness{spec.target, spec.peak, spec.stats})) return r;
    if (spec.target != 0.f && !has_out) return set_error(GSV_E_ARG, "loudness target on an item without `out`");
    if (spec.target != 0.f && n_in > LD_MAX_N) return set_error(GSV_E_ARG, "loudness: more than 640 * 4096 samples");
    if (int r = check_join(spec)) return r;
    if (join_active(spec) && !has_out) return set_error(GSV_E_ARG, "pause or trim on an item without `out`");
    if (spec.trim != 0.f && n_in > JN_MAX_N) return set_error(GSV_E_ARG, "trim: more than 640 * 4096 samples");
    return 0;
}

// The output stage alone on one buffer, its arguments checked first; spec: null, or the target to bring
// it to (needed when `target`) and the join options.  (A missing `out` is reported below as a null buffer.)
static int audio_entry(gsv_engine* eng, const float* audio_32k, int32_t n_in, const gsv_join* spec, bool target,
                       int32_t out_rate, int32_t out_format, void* out, void* stream) {
    if (!eng) return set_error(GSV_E_ARG, "null engine");
    const int rate = audio_rate_index(out_rate), n_out = gsv_audio_samples(n_in, out_rate);
    if (rate < 0 || n_out < 0) return set_error(GSV_E_ARG, "out_rate: 8000, 16000, 22050, 24000, 32000, 44100 or 48000");
    if (out_format < 0 || out_format > 1) return set_error(GSV_E_ARG, "out_format: 0 (float32) or 1 (int16)");
    if (spec) {
        if (target && spec->target == 0.f) return set_error(GSV_E_ARG, "loudness target: -50 .. -5 LUFS");
        if (int r = check_spec(*spec, true, n_in)) return r;
    }
    if (n_in > 0 && (!audio_32k || !out)) return set_error(GSV_E_ARG, "null audio buffer");
    if (spec && spec->pause != 0.f && !out) return set_error(GSV_E_ARG, "null audio buffer");
    hipSetDevice(eng->device);
    StreamScope sc(eng, stream);
    const AudioOutItem a{audio_32k, out, n_in, n_out, rate, out_format, nullptr};
    return eng->audio_out(&a, spec, 1, gsv_engine::AO_SYNC, sc.st());
}

extern "C" int gsv_audio_convert(gsv_engine* eng, const float* audio_32k, int32_t n_in, int32_t out_rate,
                                 int32_t out_format, void* out, void* stream) {
    return audio_entry(eng, audio_32k, n_in, nullptr, false, out_rate, out_format, out, stream);
}

extern "C" int gsv_audio_normalize(gsv_engine* eng, const float* audio_32k, int32_t n_in, float target, float peak,
                                   int32_t out_rate, int32_t out_format, void* out, float* stats, void* stream) {
    const gsv_join spec{target, peak, stats, 0.f, 0.f, nullptr};
    return audio_entry(eng, audio_32k, n_in, &spec, true, out_rate, out_format, out, stream);
}

extern "C" int gsv_audio_join(gsv_engine* eng, const float* audio_32k, int32_t n_in, const gsv_join* join,
                              int32_t out_rate, int32_t out_format, void* out, void* stream) {
    return audio_entry(eng, audio_32k, n_in, join, false, out_rate, out_format, out, stream);
}
