// CPU build of the filter with its feedback (csrc/mcpt_denoise.h: dn::feedback_pixel) and of the accumulation it feeds
// (csrc/mcpt_temporal.h: tp::accumulate_pixel), for tests/test_feedback_cpu.py and tests/test_gpu_feedback.py.  Compiled into a shared
// library with g++ -std=c++17 -O2 -ffp-contract=off; the frame loop mirrors launch_denoise_feedback (csrc/mcpt_denoise.hip): prep ->
// iterations with ping-pong, the feedback behind iteration k -> remodulation, every pixel through the same header functions as the kernels.
#include <cstddef>
#include <vector>

#include "mcpt_temporal.h"  // (brings mcpt_denoise.h)

using namespace mcpt;

extern "C" {

// 0 on success, 1 (MCPT_ERR_ARG) for options out of range, a bad frame size or a feedback the options do not allow.  k 0: the filter alone
// (fb_color and fb_variance untouched).  fb_variance and rec_k (the W*H records after iteration k, 8 floats each) may be null.
int fb_denoise(int W, int H, const float *color, const float *variance, const float *aov, const mcpt_denoise_opts *opts,
               const mcpt_feedback_opts *feedback, float *out, float *fb_color, float *fb_variance, float *rec_k) {
    dn::Opts o;
    int k = 0;
    if (!opts || W <= 0 || H <= 0 || dn::resolve_opts(*opts, o) != 0 || dn::resolve_feedback(feedback, o, k) != 0) return 1;
    if (k > 0 && !fb_color) return 1;
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
        if (i + 1 == k) {
            for (size_t m = 0; m < n_px; ++m) dn::feedback_pixel(m, nx[m], color, variance, aov, fb_color, fb_variance);
            if (rec_k) memcpy(rec_k, nx.data(), n_px * sizeof(dn::Rec));
        }
    }
    const std::vector<dn::Rec> &fin = rec[o.iterations & 1];
    for (size_t m = 0; m < n_px; ++m) dn::remod_pixel(m, fin[m], color, aov, out);
    return 0;
}

// tp::accumulate_pixel over a frame (tests/native/sequence_driver.cpp): 0 on success, 1 for options out of range or a bad frame size
int fb_accumulate(int W, int H, const float *color, const float *variance, const float *motion, const float *prev_color, const float *prev_variance,
                  const float *prev_depth, const float *prev_len, const mcpt_temporal_opts *opts, float *out_color, float *out_variance, float *out_len) {
    tp::Opts o;
    if (!opts || W <= 0 || H <= 0 || tp::resolve_opts(*opts, o) != 0) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel(W, H, i, j, color, variance, motion, prev_color, prev_variance, prev_depth, prev_len, o, out_color, out_variance, out_len);
    return 0;
}

}  // extern "C"
