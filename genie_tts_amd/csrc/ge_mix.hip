// Timbre fusion (include/genie_engine.h, gsv_ge_mix): the weighted sum of the global embeddings
// of several reference clips, GPT-SoVITS's auxiliary references (SynthesizerTrn.decode with a list
// of references averages the per-clip ge).  It runs once per reference set and weights; the
// result is the ge every vocoder entry already takes, so nothing on the sentence path moves.
#include <cmath>

#include "engine_internal.h"

using namespace gsv;

namespace {

// The clips' pointers and weights travel by value in the launch's arguments (192 bytes): the
// caller's host arrays need not outlive the call and there is no workspace.
struct GeMixArgs {
    const float* ge[GSV_MIX_MAX];
    float w[GSV_MIX_MAX];
};
static_assert(sizeof(GeMixArgs) == 192, "k_ge_mix's argument struct");

constexpr int GE_MIX_BLOCK = 256;

// One thread per element: acc = w_0 * x_0; acc = acc + w_i * x_i in clip order.  Every multiply
// and add is rounded on its own (contraction off, as in k_interp_linear), so a numpy restatement
// with float32 operations gives the same bits.  A thread reads its element of every input before
// it writes, and no other thread touches that element, so `out` may be one of the inputs.
__global__ __launch_bounds__(GE_MIX_BLOCK) void k_ge_mix(GeMixArgs a, int n, int dim, float* out) {
#pragma clang fp contract(off)
    const int d = blockIdx.x * GE_MIX_BLOCK + (int)threadIdx.x;
    if (d >= dim) return;
    float acc = a.w[0] * a.ge[0][d];
#pragma unroll
    for (int i = 1; i < GSV_MIX_MAX; ++i) {
        if (i >= n) break;
        const float p = a.w[i] * a.ge[i][d];
        acc = acc + p;
    }
    out[d] = acc;
}

}  // namespace

extern "C" int gsv_ge_mix(gsv_engine* eng, int32_t n, int32_t dim, const float* const* ge, const float* weights,
                          float* out, void* stream) {
    if (!eng) return set_error(GSV_E_ARG, "null engine");
    if (n < 1 || n > GSV_MIX_MAX) return set_error(GSV_E_ARG, "ge mix: n outside 1 .. " + std::to_string(GSV_MIX_MAX));
    if (dim < 1 || dim > 4096) return set_error(GSV_E_ARG, "ge mix: dim outside 1 .. 4096");
    if (!ge || !weights || !out) return set_error(GSV_E_ARG, "ge mix: null argument");
    GeMixArgs a{};
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (!ge[i]) return set_error(GSV_E_ARG, "ge mix: null embedding " + std::to_string(i));
        if (!std::isfinite(weights[i]) || weights[i] < 0.f)
            return set_error(GSV_E_ARG, "ge mix: weight " + std::to_string(i) + " is not finite and >= 0");
        any = any || weights[i] > 0.f;
        a.ge[i] = ge[i];
        a.w[i] = weights[i];
    }
    if (!any) return set_error(GSV_E_ARG, "ge mix: no weight above 0");
    hipSetDevice(eng->device);
    StreamScope sc(eng, stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ge_mix, dim3((unsigned)((dim + GE_MIX_BLOCK - 1) / GE_MIX_BLOCK)), dim3(GE_MIX_BLOCK), 0,
                       sc.st(), a, (int)n, (int)dim, out);
    return hipGetLastError() == hipSuccess ? 0 : set_error(GSV_E_HIP, "ge mix launch");
}
