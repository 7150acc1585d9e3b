// CPU build of the moments flavour of the accumulation (csrc/mcpt_temporal.h: tp::accumulate_pixel_moments) and of the variance from the
// moments (csrc/mcpt_moments.h: mo::variance_pixel), for tests/test_moments_cpu.py and tests/test_gpu_moments.py.  Compiled into a shared
// library with g++ -std=c++17 -O2 -ffp-contract=off; the frame loops mirror k_temporal_accumulate and k_moments_variance, every pixel
// through the same header function as the kernels.
#include <cstddef>

#include "mcpt_moments.h"

using namespace mcpt;

extern "C" {

// 0 on success, 1 (MCPT_ERR_ARG) for options out of range, a null array or a bad frame size.  normal / prev_normal: W*H*3, nullable unless
// the normal test is on; out_flags nullable.  Moments: W*H*2.
int mo_accumulate(int W, int H, const float *color, const float *motion, const float *normal, const float *prev_color, const float *prev_depth,
                  const float *prev_len, const float *prev_normal, const float *prev_moments, const mcpt_temporal_opts *opts,
                  const mcpt_history_opts *hopts, float *out_color, float *out_len, uint8_t *out_flags, float *out_moments) {
    tp::Opts o;
    tp::HistOpts ho;
    if (!color || !motion || !prev_color || !prev_depth || !prev_len || !prev_moments || !opts || !hopts || !out_color || !out_len || !out_moments) return 1;
    if (W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0 || tp::resolve_history_opts(*hopts, ho) != 0) return 1;
    if (ho.normal_test && (!normal || !prev_normal)) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel_moments(W, H, i, j, color, motion, normal, 3, prev_color, prev_depth, prev_len, prev_normal, prev_moments, o, ho, out_color,
                                         out_len, out_flags, out_moments);
    return 0;
}

// flags nullable.  aov: W*H*8.
int mo_variance(int W, int H, const float *moments, const float *len, const uint8_t *flags, const float *aov, const mcpt_moments_opts *opts, float *out) {
    mo::Opts o;
    if (!moments || !len || !aov || !opts || !out) return 1;
    if (W <= 0 || H <= 0 || mo::resolve_opts(*opts, o) != 0) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) out[(size_t)j * W + i] = mo::variance_pixel(W, H, i, j, moments, len, flags, aov, o);
    return 0;
}

// the resolved options {min_len, radius} and {sigma_z}; 0 on success, 1 if out of range
int mo_resolve(const mcpt_moments_opts *opts, int *ints, float *values) {
    mo::Opts o;
    if (mo::resolve_opts(*opts, o) != 0) return 1;
    ints[0] = (int)o.min_len;
    ints[1] = o.radius;
    values[0] = o.sigma_z;
    return 0;
}

}  // extern "C"
