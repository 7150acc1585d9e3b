// CPU build of the guide of an adaptive sequence (csrc/mcpt_temporal.h: tp::history_len_pixel, tp::guided_threshold), for
// tests/test_adaptive_sequence_cpu.py and tests/test_gpu_adaptive_guided.py.  Compiled into a shared library with g++ -std=c++17 -O2
// -ffp-contract=off; the frame loop mirrors k_history_len (csrc/mcpt_temporal.hip), every pixel through the same header function as the
// kernel.  tp_accumulate_ex_len is tp::accumulate_pixel_ex over the same frame, whose out_len the guide must equal wherever the new
// colour is finite.
#include <cstddef>

#include "mcpt_temporal.h"

using namespace mcpt;

extern "C" {

// 0 on success, 1 (MCPT_ERR_ARG) for options out of range, a null array or a bad frame size.  normal / prev_normal: W*H*3, nullable unless
// the normal test is on; hopts nullable (both switches off).
int tp_history_len(int W, int H, const float *motion, const float *normal, const float *prev_color, const float *prev_depth, const float *prev_len,
                   const float *prev_normal, const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts, float *len) {
    tp::Opts o;
    tp::HistOpts ho{};
    if (!motion || !prev_color || !prev_depth || !prev_len || !opts || !len) return 1;
    if (W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0 || (hopts && tp::resolve_history_opts(*hopts, ho) != 0)) return 1;
    if (ho.normal_test && (!normal || !prev_normal)) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            len[(size_t)j * W + i] = tp::history_len_pixel(W, H, i, j, motion, normal, 3, prev_color, prev_depth, prev_len, prev_normal, o, ho);
    return 0;
}

// out_len of tp::accumulate_pixel_ex (colour, variance and flags go to scratch the caller passes: W*H*3, W*H floats)
int tp_accumulate_ex_len(int W, int H, const float *color, const float *variance, const float *motion, const float *normal, const float *prev_color,
                         const float *prev_variance, const float *prev_depth, const float *prev_len, const float *prev_normal, const mcpt_temporal_opts *opts,
                         const mcpt_history_opts *hopts, float *scratch_color, float *scratch_variance, float *out_len) {
    tp::Opts o;
    tp::HistOpts ho;
    if (W <= 0 || H <= 0 || !opts || !hopts || tp::resolve_opts(*opts, o) != 0 || tp::resolve_history_opts(*hopts, ho) != 0) return 1;
    if (ho.normal_test && (!normal || !prev_normal)) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel_ex(W, H, i, j, color, variance, motion, normal, 3, prev_color, prev_variance, prev_depth, prev_len, prev_normal, o, ho,
                                    scratch_color, scratch_variance, out_len, nullptr);
    return 0;
}

// out[k] = tp::guided_threshold(threshold, guide[k])
void tp_guided_threshold(double threshold, int n, const float *guide, double *out) {
    for (int k = 0; k < n; ++k) out[k] = tp::guided_threshold(threshold, guide[k]);
}

}  // extern "C"
