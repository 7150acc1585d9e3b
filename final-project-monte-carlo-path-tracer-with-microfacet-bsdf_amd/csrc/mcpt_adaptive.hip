// Adaptive sampling: the selection step between the rounds of mcpt_render_adaptive (csrc/mcpt_render.hip).
//
// A round renders every active pixel up to n samples (round 0: n = S0 for every owned pixel; later rounds: samples [n/2, n) of the
// pixels that continued, divisor n).  Then:
//   k_adapt_eval    one lane per active pixel: the estimate e from the double moments that k_accumulate<true> summed, written to the
//                   error map, and a mark in a W x H byte image: (round stamp << 1) | (e > threshold).  k_adapt_eval<true> is the
//                   guided flavour (mcpt_render_adaptive_guided): the pixel's threshold is tp::guided_threshold(threshold, guide[m]);
//                   without a guide the plain flavour is launched, as it always was.  k_adapt_eval<2> is the weight mode
//                   (mcpt_render_adaptive_weighted): the plane holds history weights H and the pixel's threshold is
//                   threshold * sqrt((double)tp::weight_guide(H[m], n, max_history)), the Neff the weighted blend will use if the pixel
//                   stops at its n samples
//   k_adapt_select  one lane per active pixel: continue iff the pixel's own mark is set or (dilate) a neighbour's mark of THIS round is,
//                   and 2n <= spp; a continuing pixel's framebuffer value is halved (exact: DESIGN.md, adaptive sampling) and its
//                   count becomes 2n
//   adapt_compact   the continuing pixels, in list order, with their sky-cull candidate entries (hipcub::DeviceSelect::Flagged)
// The estimate follows include/mcpt.h to the letter, in double with -ffp-contract=off, so that a numpy float64 restatement of the same
// expressions decides every pixel alike.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "mcpt_adaptive.h"
#include "mcpt_temporal.h"

namespace mcpt {

namespace {

constexpr int kB = 256;
inline uint32_t nblocks(uint32_t n) { return (n + kB - 1) / kB; }

__global__ __launch_bounds__(kB) void k_sky_moments(const uint32_t *__restrict__ sky_pixels, uint32_t n_sky, float3 background, int32_t spp,
                                                     double *__restrict__ moments) {
    const uint32_t g = blockIdx.x * kB + threadIdx.x;
    if (g >= n_sky * 3u) return;
    const uint32_t m = sky_pixels[g / 3u], c = g % 3u;
    const double v = (double)(c == 0 ? background.x : (c == 1 ? background.y : background.z));
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < spp; ++k) {
        s1 += v;
        s2 += v * v;
    }
    moments[(size_t)m * 6 + c] = s1;
    moments[(size_t)m * 6 + 3 + c] = s2;
}

// m = s1/n;  q = s2/n - m*m;  var = max(q, 0) * n / (n - 1);  e_c = sqrt(var / n) / (m + rel_floor);  e = max over c, NaN if any e_c is
__device__ __forceinline__ double estimate(const double *mo, double n, double rel_floor) {
    double e = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double m = mo[c] / n;
        const double q = mo[3 + c] / n - m * m;
        const double var = (q < 0.0 ? 0.0 : q) * n / (n - 1.0);  // (a NaN q stays NaN)
        const double ec = sqrt(var / n) / (m + rel_floor);
        e = (c == 0 || ec > e || ec != ec) ? ec : e;  // (a NaN e stays NaN: no comparison with it is true)
    }
    return e;
}

enum : int { kGuideNone = 0, kGuideFrames = 1, kGuideWeight = 2 };

template <int kGuide>
__global__ __launch_bounds__(kB) void k_adapt_eval(const uint32_t *__restrict__ list, uint32_t n_list, const double *__restrict__ moments, int32_t n,
                                                    double rel_floor, double threshold, const float *__restrict__ guide, float max_history,
                                                    uint32_t round_stamp, float *__restrict__ err, uint8_t *__restrict__ stamp, int32_t *__restrict__ spp_map) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t m = list[i];
    const double e = estimate(moments + (size_t)m * 6, (double)n, rel_floor);
    err[m] = (float)e;
    spp_map[m] = n;
    const double thr = kGuide == kGuideFrames   ? tp::guided_threshold(threshold, guide[m])
                       : kGuide == kGuideWeight ? threshold * sqrt((double)tp::weight_guide(guide[m], n, max_history))
                                                : threshold;
    if (stamp) stamp[m] = (uint8_t)((round_stamp << 1) | (e > thr ? 1u : 0u));
}

__global__ __launch_bounds__(kB) void k_adapt_select(const uint32_t *__restrict__ list, uint32_t n_list, int W, int H, const uint8_t *__restrict__ stamp,
                                                      uint32_t round_stamp, int dilate, int can_double, int32_t n, float *__restrict__ fb,
                                                      int32_t *__restrict__ spp_map, uint8_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t m = list[i];
    const uint8_t hot = (uint8_t)((round_stamp << 1) | 1u);
    bool go = stamp[m] == hot;
    if (!go && dilate) {
        const int x = (int)(m % (uint32_t)W), y = (int)(m / (uint32_t)W);
        for (int dy = -1; dy <= 1 && !go; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx, yy = y + dy;
                if ((dx == 0 && dy == 0) || xx < 0 || yy < 0 || xx >= W || yy >= H) continue;
                if (stamp[(size_t)yy * W + xx] == hot) {
                    go = true;
                    break;
                }
            }
    }
    go = go && can_double;
    if (go) {
        for (int c = 0; c < 3; ++c) fb[(size_t)m * 3 + c] *= 0.5f;
        spp_map[m] = 2 * n;
    }
    flags[i] = go ? 1 : 0;
}

}  // namespace

void launch_sky_moments(const uint32_t *sky_pixels, uint32_t n_sky, const float background[3], int32_t spp, double *moments, hipStream_t st) {
    if (n_sky == 0) return;
    hipLaunchKernelGGL(k_sky_moments, dim3(nblocks(n_sky * 3u)), dim3(kB), 0, st, sky_pixels, n_sky, make_float3(background[0], background[1], background[2]),
                       spp, moments);
}

void launch_adapt_eval(const uint32_t *list, uint32_t n_list, const double *moments, int32_t n, double rel_floor, double threshold, const float *guide,
                       float weight_max_history, uint32_t round_stamp, float *err, uint8_t *stamp, int32_t *spp_map, hipStream_t st) {
    if (n_list == 0) return;
    const auto k = !guide ? k_adapt_eval<kGuideNone> : (weight_max_history > 0.f ? k_adapt_eval<kGuideWeight> : k_adapt_eval<kGuideFrames>);
    hipLaunchKernelGGL(k, dim3(nblocks(n_list)), dim3(kB), 0, st, list, n_list, moments, n, rel_floor, threshold, guide, weight_max_history, round_stamp, err,
                       stamp, spp_map);
}

void launch_adapt_select(const uint32_t *list, uint32_t n_list, int width, int height, const uint8_t *stamp, uint32_t round_stamp, int dilate,
                         int can_double, int32_t n, float *fb, int32_t *spp_map, uint8_t *flags, hipStream_t st) {
    if (n_list == 0) return;
    hipLaunchKernelGGL(k_adapt_select, dim3(nblocks(n_list)), dim3(kB), 0, st, list, n_list, width, height, stamp, round_stamp, dilate, can_double, n,
                       fb, spp_map, flags);
}

hipError_t adapt_compact(const uint32_t *list, const int4 *cand, const uint8_t *flags, uint32_t n, uint32_t *out, int4 *cand_out, void *d_temp,
                         size_t temp_bytes, uint32_t *d_count, uint32_t *n_out, hipStream_t st) {
    hipError_t e = hipcub::DeviceSelect::Flagged(d_temp, temp_bytes, list, flags, out, d_count, (int)n, st);
    if (e == hipSuccess && cand) e = hipcub::DeviceSelect::Flagged(d_temp, temp_bytes, cand, flags, cand_out, d_count, (int)n, st);  // the same order
    uint32_t cnt = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&cnt, d_count, sizeof cnt, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    *n_out = cnt;
    return hipSuccess;
}

size_t adapt_temp_bytes(uint32_t n) {
    size_t a = 0, b = 0;
    (void)hipcub::DeviceSelect::Flagged(nullptr, a, (const uint32_t *)nullptr, (const uint8_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n);
    (void)hipcub::DeviceSelect::Flagged(nullptr, b, (const int4 *)nullptr, (const uint8_t *)nullptr, (int4 *)nullptr, (uint32_t *)nullptr, (int)n);
    return a > b ? a : b;
}

}  // namespace mcpt
