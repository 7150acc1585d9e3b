// CPU build of the accumulation with history rejection (csrc/mcpt_temporal.h: tp::accumulate_pixel_ex), for tests/test_history_cpu.py and
// tests/test_gpu_history.py.  Compiled into a shared library with g++ -std=c++17 -O2 -ffp-contract=off; the frame loop mirrors
// k_temporal_accumulate (csrc/mcpt_temporal.hip), every pixel through the same header function as the kernel.  tp_accumulate_plain is
// tp::accumulate_pixel, what the _ex function must equal with both switches off.
#include <cstddef>

#include "mcpt_temporal.h"

using namespace mcpt;

extern "C" {

// 0 on success, 1 (MCPT_ERR_ARG) for options out of range, a null array or a bad frame size.  normal / prev_normal: W*H*3, nullable unless
// the normal test is on; out_flags nullable.
int tp_accumulate_ex(int W, int H, const float *color, const float *variance, const float *motion, const float *normal, const float *prev_color,
                     const float *prev_variance, const float *prev_depth, const float *prev_len, const float *prev_normal, const mcpt_temporal_opts *opts,
                     const mcpt_history_opts *hopts, float *out_color, float *out_variance, float *out_len, uint8_t *out_flags) {
    tp::Opts o;
    tp::HistOpts ho;
    if (!color || !variance || !motion || !prev_color || !prev_variance || !prev_depth || !prev_len || !opts || !hopts || !out_color || !out_variance ||
        !out_len)
        return 1;
    if (W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0 || tp::resolve_history_opts(*hopts, ho) != 0) return 1;
    if (ho.normal_test && (!normal || !prev_normal)) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel_ex(W, H, i, j, color, variance, motion, normal, 3, prev_color, prev_variance, prev_depth, prev_len, prev_normal, o, ho,
                                    out_color, out_variance, out_len, out_flags);
    return 0;
}

int tp_accumulate_plain(int W, int H, const float *color, const float *variance, const float *motion, const float *prev_color, const float *prev_variance,
                        const float *prev_depth, const float *prev_len, const mcpt_temporal_opts *opts, float *out_color, float *out_variance,
                        float *out_len) {
    tp::Opts o;
    if (W <= 0 || H <= 0 || !opts || tp::resolve_opts(*opts, o) != 0) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel(W, H, i, j, color, variance, motion, prev_color, prev_variance, prev_depth, prev_len, o, out_color, out_variance, out_len);
    return 0;
}

// the resolved options {normal_test, color_clamp} and {normal_min, clamp_k}; 0 on success, 1 if out of range
int tp_resolve_history(const mcpt_history_opts *hopts, int *switches, float *values) {
    tp::HistOpts ho;
    if (tp::resolve_history_opts(*hopts, ho) != 0) return 1;
    switches[0] = ho.normal_test;
    switches[1] = ho.color_clamp;
    values[0] = ho.normal_min;
    values[1] = ho.clamp_k;
    return 0;
}

}  // extern "C"
