/*
 * mcpt_moments.h -- the variance of an accumulated frame from the temporal moments of its luminance (include/mcpt.h: mcpt_moments_variance).
 *
 * The temporal half of SVGF (Schied et al. 2017): a sequence at one sample per pixel has no per-frame variance, so the history carries the
 * running first and second moment of each pixel's luminance (the kMoments flavour of tp::reuse_pixel, csrc/mcpt_temporal.h) and the variance
 * the filter is guided by comes from them: temporally where the history is long enough, from a gated spatial window of the moments where
 * it is not.  Every function here is callable from the host and from the device, and both compilations (hipcc -ffp-contract=off for gfx950;
 * g++ -std=c++17 -O2 -ffp-contract=off) give the same bits: float32 arithmetic in a fixed order, no FMA, correctly rounded f32 division.
 * tests/test_moments_cpu.py checks the host build against a numpy restatement and tests/test_gpu_moments.py checks the device against the
 * host build bit for bit.  csrc/mcpt_moments.hip holds the kernel.
 */
#ifndef MCPT_MOMENTS_H
#define MCPT_MOMENTS_H

#include "mcpt_temporal.h"  // (brings mcpt_denoise.h: dn::depth_gradient, and tp::load_moments)

#if defined(__HIPCC__) || defined(__HIP__)
#define MCPT_MO static __host__ __device__ __forceinline__
#else
#include <math.h>
#define MCPT_MO static inline
#endif

namespace mcpt {
namespace mo {

constexpr int32_t kMaxRadius = 4;  // a 9 x 9 window: 81 taps

// Options after the defaults of include/mcpt.h have been applied.
struct Opts {
    float min_len;  // 2..4096, an integer value
    int32_t radius;  // 1..4
    float sigma_z;   // > 0, finite
};

// 0 on success, -1 if an option is out of range (enabled included: 0 or 1).
MCPT_MO int resolve_opts(const mcpt_moments_opts &o, Opts &out) {
    for (int k = 0; k < 4; ++k)
        if (o.reserved[k] != 0) return -1;
    if (o.enabled != 0 && o.enabled != 1) return -1;
    const int32_t ml = o.min_len == 0 ? 4 : o.min_len;
    if (ml < 2 || ml > tp::kMaxHistory) return -1;
    const int32_t r = o.radius == 0 ? 3 : o.radius;
    if (r < 1 || r > kMaxRadius) return -1;
    const float sz = o.sigma_z == 0.0f ? 1.0f : o.sigma_z;
    if (!(sz > 0.0f && sz <= 3.0e38f)) return -1;  // (positive and finite; NaN fails)
    out.min_len = (float)ml;
    out.radius = r;
    out.sigma_z = sz;
    return 0;
}

MCPT_MO bool finite_f(float x) { return x - x == 0.0f; }  // false for +-inf and NaN

/* The variance of the accumulated colour's luminance at pixel (x, y) of a W x H frame, from the moments the accumulation left (2 floats per
 * pixel, interleaved), its history lengths len, its flags (nullable: no pixel is clamped) and the AOV records the filter will read (8 floats
 * per pixel).  With (mu1, mu2) the pixel's moments, N = len[p] and clamped = flags && (flags[p] & 2):
 *   the pixel's own moments are not finite (its colour was not): +inf, which the filter passes through;
 *   temporal branch, N >= min_len and not clamped:
 *       q = mu2 - mu1*mu1;  q = q > 0 ? q : 0;  v = q / (N - 1.f)
 *     -- the unbiased per-frame variance q N / (N - 1) over the N frames of a running mean.  Beyond max_history the mean is exponential and
 *     its variance smaller: an over-estimate, so the filter smooths more, never less;
 *   spatial branch, everything else (a short history, a clamped one): over the window dy = -r..r (outer), dx = -r..r, the pixel itself
 *     included, a pixel q counts if it is in the image, its moments are finite and it passes a binary gate built from the filter's own
 *     expressions: both uncovered; or both covered (coverage > 0) with n_p.n_q > 0 (x + (y + z), dn::same_surface's order) and
 *       |z_p - z_q| <= (sigma_z |grad_p . (dx, dy)| + 1e-3 max(z_p, z_q)) + 1e-6,   grad_p = dn::depth_gradient.
 *     A gate, not the filter's max(0, n.n)^sigma_n: a short folded normal would make such weights subnormal and the mean 0 / 0.
 *       cnt = cnt + 1.f;  s1 = s1 + mu1_q;  s2 = s2 + mu2_q;   then   a = s1 / cnt;  b = s2 / cnt;  q = b - a*a;  q = q > 0 ? q : 0;
 *       sig2 = q * (cnt / (cnt - 1.f));   cnt < 2: sig2 = mu2_p (a variance never exceeds the second moment);
 *       v = sig2 / (clamped ? 1.f : N)
 *     -- a clamped history was moved to the new frame's neighbourhood: it is worth one frame. */
MCPT_MO float variance_pixel(int W, int H, int x, int y, const float *moments, const float *len, const uint8_t *flags, const float *aov, const Opts &o) {
    const size_t m = (size_t)y * W + x;
    const tp::Mom2 mp = tp::load_moments(moments, m);
    if (!(finite_f(mp.m1) && finite_f(mp.m2))) return HUGE_VALF;
    const float N = len[m];
    const bool clamped = flags && (flags[m] & 2);
    if (N >= o.min_len && !clamped) {
        const float q = mp.m2 - mp.m1 * mp.m1;
        return (q > 0.0f ? q : 0.0f) / (N - 1.0f);
    }
    const float *ap = aov + m * 8;
    const float np0 = ap[3], np1 = ap[4], np2 = ap[5], zp = ap[6];
    const bool cov_p = ap[7] > 0.0f;
    float grad[2];
    dn::depth_gradient(W, H, x, y, aov, grad);
    float cnt = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -o.radius; dy <= o.radius; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -o.radius; dx <= o.radius; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const size_t k = (size_t)yy * W + xx;
            const float *aq = aov + k * 8;
            const bool cov_q = aq[7] > 0.0f;
            if (cov_p != cov_q) continue;
            if (cov_p) {
                const float nd = np0 * aq[3] + (np1 * aq[4] + np2 * aq[5]);
                if (!(nd > 0.0f)) continue;
                const float zq = aq[6];
                const float gd = grad[0] * (float)dx + grad[1] * (float)dy;
                const float den_z = (o.sigma_z * dn::abs_f(gd) + 1e-3f * dn::max_f(zp, zq)) + 1e-6f;
                if (!(dn::abs_f(zp - zq) <= den_z)) continue;  // (a NaN depth on either side fails)
            }
            const tp::Mom2 mq = tp::load_moments(moments, k);
            if (!(finite_f(mq.m1) && finite_f(mq.m2))) continue;
            cnt = cnt + 1.0f;
            s1 = s1 + mq.m1;
            s2 = s2 + mq.m2;
        }
    }
    float sig2 = mp.m2;
    if (cnt >= 2.0f) {
        const float a = s1 / cnt, b = s2 / cnt;
        const float q = b - a * a;
        sig2 = (q > 0.0f ? q : 0.0f) * (cnt / (cnt - 1.0f));
    }
    return sig2 / (clamped ? 1.0f : N);
}

}  // namespace mo
}  // namespace mcpt

#undef MCPT_MO

#if defined(__HIPCC__) || defined(__HIP__)
namespace mcpt {
// Launcher of csrc/mcpt_moments.hip (asynchronous on `st`): out[m] = mo::variance_pixel for every pixel of a W x H frame (k_moments_variance).
void launch_moments_variance(int W, int H, const mo::Opts &o, const float *moments, const float *len, const uint8_t *flags, const float *aov, float *out,
                             hipStream_t st);
}  // namespace mcpt
#endif
#endif  // MCPT_MOMENTS_H
