// CPU build of the accumulation of a frame sequence (csrc/mcpt_temporal.h: tp::accumulate_pixel), for tests/test_sequence_cpu.py and
// tests/test_gpu_sequence.py.  Compiled into a shared library with g++ -std=c++17 -O2 -ffp-contract=off; the frame loop mirrors
// k_temporal_accumulate (csrc/mcpt_temporal.hip), every pixel through the same header function as the kernel.
#include <cstddef>

#include "mcpt_temporal.h"

using namespace mcpt;

extern "C" {

// 0 on success, 1 (MCPT_ERR_ARG) for options out of range, a null array or a bad frame size
int tp_accumulate(int W, int H, const float *color, const float *variance, const float *motion, const float *prev_color, const float *prev_variance,
                  const float *prev_depth, const float *prev_len, const mcpt_temporal_opts *opts, float *out_color, float *out_variance, float *out_len) {
    tp::Opts o;
    if (!color || !variance || !motion || !prev_color || !prev_variance || !prev_depth || !prev_len || !opts || !out_color || !out_variance || !out_len)
        return 1;
    if (W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel(W, H, i, j, color, variance, motion, prev_color, prev_variance, prev_depth, prev_len, o, out_color, out_variance, out_len);
    return 0;
}

}  // extern "C"
