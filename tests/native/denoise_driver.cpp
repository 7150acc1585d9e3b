// CPU build of the denoiser's arithmetic (csrc/mcpt_denoise.h), for tests/test_denoise_cpu.py and tests/test_gpu_denoise.py.
// Compiled into a shared library with g++ -std=c++17 -O2 -ffp-contract=off; the frame loop mirrors csrc/mcpt_denoise.hip
// (prep -> iterations with ping-pong -> remodulation), every pixel through the same header functions as the kernels.
#include <cstddef>
#include <vector>

#include "mcpt_denoise.h"

using namespace mcpt;

extern "C" {

void dn_exp(long long n, const float *x, float *out) {
    for (long long i = 0; i < n; ++i) out[i] = dn::exp_f(x[i]);
}

void dn_pow_int(long long n, const float *b, int e, float *out) {
    for (long long i = 0; i < n; ++i) out[i] = dn::pow_int(b[i], e);
}

void dn_variance(long long n_px, const double *moments, int n, float *out) {
    for (long long m = 0; m < n_px; ++m) out[m] = dn::luminance_variance(moments + m * 6, moments + m * 6 + 3, (double)n);
}

// 0 on success, 1 (MCPT_ERR_ARG) for options out of range or a bad frame size
int dn_denoise(int W, int H, const float *color, const float *variance, const float *aov, const mcpt_denoise_opts *opts, float *out) {
    dn::Opts o;
    if (!opts || W <= 0 || H <= 0 || dn::resolve_opts(*opts, o) != 0) return 1;
    const size_t n_px = (size_t)W * H;
    std::vector<dn::Rec> rec[2] = {std::vector<dn::Rec>(n_px), std::vector<dn::Rec>(n_px)};
    std::vector<float> grad(n_px * 2);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) dn::prep_pixel(W, H, x, y, color, variance, aov, rec[0][(size_t)y * W + x], &grad[((size_t)y * W + x) * 2]);
    for (int i = 0; i < o.iterations; ++i) {
        const std::vector<dn::Rec> &in = rec[i & 1];
        std::vector<dn::Rec> &nx = rec[(i + 1) & 1];
        auto load = [&in](size_t q) { return in[q]; };
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) dn::atrous_pixel(W, H, x, y, 1 << i, o, load, &grad[((size_t)y * W + x) * 2], nx[(size_t)y * W + x]);
    }
    const std::vector<dn::Rec> &fin = rec[o.iterations & 1];
    for (size_t m = 0; m < n_px; ++m) dn::remod_pixel(m, fin[m], color, aov, out);
    return 0;
}

}  // extern "C"
