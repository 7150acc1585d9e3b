// CPU build of the count-weighted flavour of temporal reuse (csrc/mcpt_temporal.h: tp::accumulate_pixel_weighted, tp::history_weight_pixel,
// tp::weight_guide), for tests/test_weighted_cpu.py, tests/test_gpu_weighted.py and tests/test_gpu_sequence_weighted.py.  Compiled into a
// shared library with g++ -std=c++17 -O2 -ffp-contract=off; the frame loops mirror k_temporal_accumulate<.., .., true> and k_history_weight
// (csrc/mcpt_temporal.hip), every pixel through the same header function as the kernel.  tp_accumulate_unweighted is
// tp::accumulate_pixel_ex over the same frame, the rule the flavour must equal under uniform counts.
#include <cstddef>
#include <cstdint>

#include "mcpt_temporal.h"

using namespace mcpt;

extern "C" {

// 0 on success, 1 (MCPT_ERR_ARG) for what mcpt_temporal_accumulate_weighted refuses: options out of range, a null array, a bad frame size,
// a count below 1, or with a null count a uniform_count below 1 or not finite.  normal / prev_normal: W*H*3, nullable unless the normal test
// is on; count: W*H int32, nullable; out_flags nullable.
int tp_accumulate_weighted(int W, int H, const float *color, const float *variance, const float *motion, const float *normal, const int32_t *count,
                           float uniform_count, const float *prev_color, const float *prev_variance, const float *prev_depth, const float *prev_len,
                           const float *prev_normal, const float *prev_weight, const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts,
                           float *out_color, float *out_variance, float *out_len, uint8_t *out_flags, float *out_weight) {
    tp::Opts o;
    tp::HistOpts ho;
    if (!color || !variance || !motion || !prev_color || !prev_variance || !prev_depth || !prev_len || !prev_weight || !opts || !hopts || !out_color ||
        !out_variance || !out_len || !out_weight)
        return 1;
    if (W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0 || tp::resolve_history_opts(*hopts, ho) != 0) return 1;
    if (ho.normal_test && (!normal || !prev_normal)) return 1;
    if (count) {
        for (size_t m = 0; m < (size_t)W * H; ++m)
            if (count[m] < 1) return 1;
    } else if (!(uniform_count >= 1.0f && uniform_count <= 3.0e38f)) {
        return 1;
    }
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel_weighted(W, H, i, j, color, variance, motion, normal, 3, count, uniform_count, prev_color, prev_variance, prev_depth, prev_len,
                                          prev_normal, prev_weight, o, ho, out_color, out_variance, out_len, out_flags, out_weight);
    return 0;
}

// tp::accumulate_pixel_ex over a frame (the unweighted rule)
int tp_accumulate_unweighted(int W, int H, const float *color, const float *variance, const float *motion, const float *normal, const float *prev_color,
                             const float *prev_variance, const float *prev_depth, const float *prev_len, const float *prev_normal,
                             const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts, float *out_color, float *out_variance, float *out_len,
                             uint8_t *out_flags) {
    tp::Opts o;
    tp::HistOpts ho;
    if (W <= 0 || H <= 0 || !opts || !hopts || tp::resolve_opts(*opts, o) != 0 || tp::resolve_history_opts(*hopts, ho) != 0) return 1;
    if (ho.normal_test && (!normal || !prev_normal)) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel_ex(W, H, i, j, color, variance, motion, normal, 3, prev_color, prev_variance, prev_depth, prev_len, prev_normal, o, ho,
                                    out_color, out_variance, out_len, out_flags);
    return 0;
}

// tp::history_weight_pixel over a frame; hopts nullable (both switches off)
int tp_history_weight(int W, int H, const float *motion, const float *normal, const float *prev_color, const float *prev_depth, const float *prev_len,
                      const float *prev_normal, const float *prev_weight, const mcpt_temporal_opts *opts, const mcpt_history_opts *hopts, float *weight) {
    tp::Opts o;
    tp::HistOpts ho{};
    if (!motion || !prev_color || !prev_depth || !prev_len || !prev_weight || !opts || !weight) return 1;
    if (W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0 || (hopts && tp::resolve_history_opts(*hopts, ho) != 0)) return 1;
    if (ho.normal_test && (!normal || !prev_normal)) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            weight[(size_t)j * W + i] =
                tp::history_weight_pixel(W, H, i, j, motion, normal, 3, prev_color, prev_depth, prev_len, prev_normal, prev_weight, o, ho);
    return 0;
}

// out[k] = tp::weight_guide(H[k], n[k], max_history[k])
void tp_weight_guide(int count, const float *H, const int32_t *n, const float *max_history, float *out) {
    for (int k = 0; k < count; ++k) out[k] = tp::weight_guide(H[k], n[k], max_history[k]);
}

}  // extern "C"
