/*
 * mcpt_denoise.h -- the per-pixel and per-tap arithmetic of the guided a-trous denoiser (include/mcpt.h: mcpt_denoise).
 *
 * Dammertz et al. 2010 ("Edge-avoiding a-trous wavelet transform") with the variance guidance of SVGF (Schied et al. 2017), on the
 * demodulated colour e = colour / max(albedo, 1e-3).  Every function here is callable from the host and from the device, and both
 * compilations (hipcc -ffp-contract=off for gfx950; g++ -std=c++17 -O2 -ffp-contract=off) give the same bits: float32 arithmetic
 * in a fixed order, no FMA, correctly rounded f32 division and square root (hipcc's default), and the one transcendental, exp,
 * written out below in plain double arithmetic.  tests/test_denoise_cpu.py checks the host build against a numpy restatement and
 * tests/test_gpu_denoise.py checks the device against the host build bit for bit.  csrc/mcpt_denoise.hip holds the kernels.
 *
 * Records (32 bytes, two 16-byte loads per tap): {e.rgb, v} {n.xyz, z}.
 *   !(v >= 0)  (kInvalid = -1) the pixel's colour or variance is not usable: it passes through and is no neighbour (usable() below; a NaN
 *              v counts as unusable too, although no step of the filter forms one)
 *   z < 0   (kUncovered) no feature sample of the pixel hit anything (coverage 0); otherwise z is the mean hit distance
 */
#ifndef MCPT_DENOISE_H
#define MCPT_DENOISE_H

#include <stdint.h>
#include <string.h>

#include "../../include/mcpt.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MCPT_DN static __host__ __device__ __forceinline__
#else
#include <math.h>
#define MCPT_DN static inline
#endif

namespace mcpt {
namespace dn {

struct alignas(16) Rec {
    float e[3], v;
    float n[3], z;
};
static_assert(sizeof(Rec) == 32, "Rec must be 32 bytes");

constexpr float kInvalid = -1.0f;    // Rec::v of a pixel that passes through
constexpr float kUncovered = -1.0f;  // Rec::z of a pixel with coverage 0
constexpr float kAlbedoFloor = 1e-3f;
constexpr int kMaxIterations = 8;
constexpr int kMaxSpecularDepth = 8;  // mcpt_denoise_opts::specular_depth, mcpt_render_aovs_ex

// Options after the defaults of include/mcpt.h have been applied.
struct Opts {
    int32_t iterations;  // 1..8
    int32_t sigma_n;     // 1..1024
    float sigma_l, sigma_z;
};

// 0 on success, -1 if an option is out of range (aov_spp is checked by the callers that use it).
MCPT_DN int resolve_opts(const mcpt_denoise_opts &o, Opts &out) {
    if (o.aov_spp < 0) return -1;
    if (o.specular_depth < 0 || o.specular_depth > kMaxSpecularDepth) return -1;
    if (o.reserved[0] != 0 || o.reserved[1] != 0) return -1;
    out.iterations = o.iterations == 0 ? 5 : o.iterations;
    if (out.iterations < 1 || out.iterations > kMaxIterations) return -1;
    const float sl = o.sigma_l == 0.0f ? 4.0f : o.sigma_l, sz = o.sigma_z == 0.0f ? 1.0f : o.sigma_z;
    if (!(sl > 0.0f && sl <= 3.0e38f) || !(sz > 0.0f && sz <= 3.0e38f)) return -1;  // (positive and finite; NaN fails both)
    out.sigma_l = sl;
    out.sigma_z = sz;
    const float sn = o.sigma_n == 0.0f ? 128.0f : o.sigma_n;
    if (!(sn >= 1.0f && sn <= 1024.0f) || (float)(int32_t)sn != sn) return -1;
    out.sigma_n = (int32_t)sn;
    return 0;
}

// The iteration a feedback history is taken behind (mcpt_feedback_opts; null: 0, off), checked against the resolved options: 0 on success,
// -1 for an iteration outside 0..o.iterations or a non-zero reserved word.
MCPT_DN int resolve_feedback(const mcpt_feedback_opts *f, const Opts &o, int &k) {
    k = 0;
    if (!f) return 0;
    for (int i = 0; i < 7; ++i)
        if (f->reserved[i] != 0) return -1;
    if (f->iteration < 0 || f->iteration > kMaxIterations || f->iteration > o.iterations) return -1;
    k = f->iteration;
    return 0;
}

MCPT_DN bool finite_f(float x) { return x - x == 0.0f; }  // false for +-inf and NaN
MCPT_DN float max_f(float a, float b) { return a < b ? b : a; }
MCPT_DN float abs_f(float a) { return a < 0.0f ? -a : a; }
// luminance weights (Rec. 709)
MCPT_DN float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
MCPT_DN float albedo_floor(float a) { return a > kAlbedoFloor ? a : kAlbedoFloor; }  // max(albedo, 1e-3); a NaN albedo gives 1e-3

/* exp(x), rounded once to float.  Double arithmetic with + - * / and an int conversion only, in a fixed order: x = k ln2 + r with
 * |r| <= ln2/2 (two-part ln2: the first part has 32 significant bits, so k * part1 is exact for |k| < 2^21), exp(r) by its Taylor
 * polynomial through r^12 (truncation < 2e-16), times 2^k built from its bits.  The double result is within a few double ulps, so
 * the float is the correctly rounded value except within ~1e-8 ulp of a rounding boundary: within 1 ulp everywhere.
 * x < -87 (and NaN) returns 0, so no subnormal result ever decides a bit; x > 88 returns +inf. */
MCPT_DN float exp_f(float x) {
    if (!(x >= -87.0f)) return 0.0f;
    if (x > 88.0f) return (float)(1e300 * 1e300);
    const double xd = (double)x;
    const double kd = xd * 1.44269504088896338700e+00;
    const int32_t k = (int32_t)(kd < 0.0 ? kd - 0.5 : kd + 0.5);
    const double r = (xd - (double)k * 6.93147180369123816490e-01) - (double)k * 1.90821492927058770002e-10;
    double p = 1.0 / 479001600.0;
    p = 1.0 / 39916800.0 + r * p;
    p = 1.0 / 3628800.0 + r * p;
    p = 1.0 / 362880.0 + r * p;
    p = 1.0 / 40320.0 + r * p;
    p = 1.0 / 5040.0 + r * p;
    p = 1.0 / 720.0 + r * p;
    p = 1.0 / 120.0 + r * p;
    p = 1.0 / 24.0 + r * p;
    p = 1.0 / 6.0 + r * p;
    p = 0.5 + r * p;
    p = 1.0 + r * p;
    p = 1.0 + r * p;
    const uint64_t bits = (uint64_t)(int64_t)(k + 1023) << 52;
    double two_k;
    memcpy(&two_k, &bits, sizeof two_k);
    return (float)(p * two_k);
}

// b^n for an integer n >= 1: square-and-multiply over the bits of n from the lowest, in float
MCPT_DN float pow_int(float b, int32_t n) {
    float r = 1.0f;
    while (n > 0) {
        if (n & 1) r = r * b;
        b = b * b;
        n >>= 1;
    }
    return r;
}

/* The depth gradient of pixel (x, y) from the AOV records (8 floats per pixel: depth at 6, coverage at 7): central differences over covered
 * in-image neighbours ((z+ - z-) / 2; one-sided when one neighbour is missing; 0 when both are, and for an uncovered pixel).  prep_pixel
 * and the window gate of the moments variance (csrc/mcpt_moments.h) both take it from here. */
MCPT_DN void depth_gradient(int W, int H, int x, int y, const float *aov, float grad[2]) {
    const float *a = aov + ((size_t)y * W + x) * 8;
    const bool cov = a[7] > 0.0f;
    const float z = a[6];
    float g[2] = {0.0f, 0.0f};
    if (cov) {
        for (int axis = 0; axis < 2; ++axis) {
            const int dx = axis == 0 ? 1 : 0, dy = axis == 0 ? 0 : 1;
            const int xm = x - dx, ym = y - dy, xp = x + dx, yp = y + dy;
            const bool hm = xm >= 0 && ym >= 0 && aov[((size_t)ym * W + xm) * 8 + 7] > 0.0f;
            const bool hp = xp < W && yp < H && aov[((size_t)yp * W + xp) * 8 + 7] > 0.0f;
            const float zm = hm ? aov[((size_t)ym * W + xm) * 8 + 6] : 0.0f, zp = hp ? aov[((size_t)yp * W + xp) * 8 + 6] : 0.0f;
            g[axis] = (hm && hp) ? (zp - zm) * 0.5f : (hp ? zp - z : (hm ? z - zm : 0.0f));
        }
    }
    grad[0] = g[0];
    grad[1] = g[1];
}

/* Preparation of pixel (x, y) of a W x H frame: colour (3 floats), variance (1) and AOV record (8 floats: albedo, normal, depth,
 * coverage) per pixel, row-major.  Demodulation e = c / A, A = max(albedo, 1e-3), and v / lum(A)^2.  The pixel is usable iff c, v, e
 * and the scaled v are finite and v >= 0.  grad: the depth gradient (depth_gradient above). */
MCPT_DN void prep_pixel(int W, int H, int x, int y, const float *color, const float *variance, const float *aov, Rec &out, float grad[2]) {
    const size_t m = (size_t)y * W + x;
    const float *a = aov + m * 8;
    const float A0 = albedo_floor(a[0]), A1 = albedo_floor(a[1]), A2 = albedo_floor(a[2]);
    const float c0 = color[m * 3], c1 = color[m * 3 + 1], c2 = color[m * 3 + 2];
    const float v = variance[m];
    const float e0 = c0 / A0, e1 = c1 / A1, e2 = c2 / A2;
    const float la = lum(A0, A1, A2);
    const float vs = v / (la * la);
    const bool ok = finite_f(c0) && finite_f(c1) && finite_f(c2) && finite_f(v) && v >= 0.0f && finite_f(e0) && finite_f(e1) && finite_f(e2) &&
                    finite_f(vs);
    out.e[0] = ok ? e0 : 0.0f;
    out.e[1] = ok ? e1 : 0.0f;
    out.e[2] = ok ? e2 : 0.0f;
    out.v = ok ? vs : kInvalid;
    out.n[0] = a[3];
    out.n[1] = a[4];
    out.n[2] = a[5];
    out.z = a[7] > 0.0f ? a[6] : kUncovered;
    depth_gradient(W, H, x, y, aov, grad);
}

/* Whether q may contribute to p at all: q is usable, and both are uncovered or both covered with n_p.n_q > 0.  The taps' weights are 0
 * otherwise, and the prefilter of v skips such neighbours too, so that nothing -- not even the variance, which the iterations update
 * from the colours -- crosses a coverage seam or a seam of orthogonal or opposed normals. */
MCPT_DN bool usable(const Rec &r) { return r.v >= 0.0f; }  // false for kInvalid and for NaN

MCPT_DN bool same_surface(const Rec &p, const Rec &q) {
    if (!usable(q)) return false;
    const bool cp = p.z >= 0.0f, cq = q.z >= 0.0f;
    if (cp != cq) return false;
    return !cp || p.n[0] * q.n[0] + (p.n[1] * q.n[1] + p.n[2] * q.n[2]) > 0.0f;
}

/* One a-trous iteration at pixel (x, y), step s = 2^i.  in: the W x H records of the previous iteration (the prepared ones for i = 0);
 * grad: the pixel's depth gradient.  Writes the pixel's new record (an unusable pixel, or one whose weights sum to 0, keeps its record):
 *   g_p  = the (1,2,1)^2 prefilter of v over the in-image pixels q of the 3 x 3 neighbourhood with same_surface(p, q), divided by the
 *          weights it used (p itself always takes part unless n_p = 0)
 *   taps q = p + s (dx, dy), dy = -2..2 (outer), dx = -2..2, in image and usable:
 *        w = h(dx) h(dy) * max(0, n_p.n_q)^sigma_n * exp(-(|z_p - z_q| / (sigma_z |grad_p . (s dx, s dy)| + 1e-3 max(z_p, z_q) + 1e-6)
 *                                                       + |l_p - l_q| / (sigma_l sqrt(g_p) + 1e-6)))
 *        h = (1/16, 1/4, 3/8, 1/4, 1/16), l = lum(e); one of p, q uncovered: w = 0; both uncovered: the normal and depth terms are 1
 *   e'_p = sum (w / sum w) e_q,  v'_p = sum (w / sum w)^2 v_q  (= sum w e_q / sum w and sum w^2 v_q / (sum w)^2, in a form that keeps
 *   its precision: the weights of a pixel whose folded normal is short -- an edge pixel whose feature samples split between two surfaces
 *   -- are tiny, down to subnormal, so w e_q would lose its bits and (sum w)^2 would round to 0.  A second pass over the 25 taps, whose
 *   weights stay in registers, normalises them first and reads {e_q, v_q} again (from cache); taps of weight 0 add nothing.) */
template <typename Load>
MCPT_DN void atrous_pixel(int W, int H, int x, int y, int step, const Opts &o, const Load &load, const float grad[2], Rec &out) {
    const Rec p = load((size_t)y * W + x);
    out = p;
    if (!usable(p)) return;
    float sk = 0.0f, sv = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const Rec q = (dx == 0 && dy == 0) ? p : load((size_t)yy * W + xx);
            if (!same_surface(p, q)) continue;
            const float vq = q.v;
            const float k = (dx == 0 ? 2.0f : 1.0f) * (dy == 0 ? 2.0f : 1.0f);
            sk = sk + k;
            sv = sv + k * vq;
        }
    }
    const float g = sk > 0.0f ? sv / sk : 0.0f;
    const float den_l = o.sigma_l * sqrtf(g) + 1e-6f;
    const float lp = lum(p.e[0], p.e[1], p.e[2]);
    const bool cov_p = p.z >= 0.0f;
    const float h[5] = {1.0f / 16.0f, 0.25f, 0.375f, 0.25f, 1.0f / 16.0f};
    float sw = 0.0f;
    float wk[25];  // per tap (dy-major): the weight, 0 for skipped taps
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dy = -2; dy <= 2; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int dx = -2; dx <= 2; ++dx) {
            const int t = (dy + 2) * 5 + (dx + 2);
            wk[t] = 0.0f;
            const int yy = y + step * dy, xx = x + step * dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const Rec q = (dx == 0 && dy == 0) ? p : load((size_t)yy * W + xx);
            if (!usable(q)) continue;
            const bool cov_q = q.z >= 0.0f;
            if (cov_p != cov_q) continue;
            float w = h[dx + 2] * h[dy + 2];
            const float lq = lum(q.e[0], q.e[1], q.e[2]);
            float arg = abs_f(lp - lq) / den_l;
            if (cov_p) {
                const float nd = p.n[0] * q.n[0] + (p.n[1] * q.n[1] + p.n[2] * q.n[2]);
                w = w * pow_int(nd > 0.0f ? nd : 0.0f, o.sigma_n);
                const float gd = grad[0] * (float)(step * dx) + grad[1] * (float)(step * dy);
                const float den_z = (o.sigma_z * abs_f(gd) + 1e-3f * max_f(p.z, q.z)) + 1e-6f;
                arg = abs_f(p.z - q.z) / den_z + arg;
            }
            w = w * exp_f(-arg);
            wk[t] = w;
            sw = sw + w;
        }
    }
    if (!(sw > 0.0f)) return;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 25; ++t) {
        if (!(wk[t] > 0.0f)) continue;  // (adding 0 would not change a sum: skipping it keeps the bits and stays inside the image)
        const int dy = t / 5 - 2, dx = t % 5 - 2;
        const Rec q = (dx == 0 && dy == 0) ? p : load((size_t)(y + step * dy) * W + (x + step * dx));
        const float wn = wk[t] / sw;
        s0 = s0 + wn * q.e[0];
        s1 = s1 + wn * q.e[1];
        s2 = s2 + wn * q.e[2];
        s3 = s3 + (wn * wn) * q.v;
    }
    out.e[0] = s0;
    out.e[1] = s1;
    out.e[2] = s2;
    out.v = s3;
}

// Remodulation of pixel m: out = e * A; an unusable pixel passes its colour through unchanged.
MCPT_DN void remod_pixel(size_t m, const Rec &r, const float *color, const float *aov, float *out) {
    const float *a = aov + m * 8;
    if (!usable(r)) {
        out[m * 3] = color[m * 3];
        out[m * 3 + 1] = color[m * 3 + 1];
        out[m * 3 + 2] = color[m * 3 + 2];
        return;
    }
    out[m * 3] = r.e[0] * albedo_floor(a[0]);
    out[m * 3 + 1] = r.e[1] * albedo_floor(a[1]);
    out[m * 3 + 2] = r.e[2] * albedo_floor(a[2]);
}

/* The history a feedback sequence keeps of pixel m (include/mcpt.h: mcpt_denoise_feedback): r is the pixel's record after a-trous iteration
 * k, 1 <= k <= iterations -- the buffer iteration k + 1 reads.  A usable record gives the colour remod_pixel would give there, e * A, and its
 * variance with the scaling of prep_pixel undone, v * lum(A)^2; an unusable one passes colour and variance through with their bits.
 * out_variance may be null (a moments sequence keeps no fed variance). */
MCPT_DN void feedback_pixel(size_t m, const Rec &r, const float *color, const float *variance, const float *aov, float *out_color,
                            float *out_variance) {
    // (every load first and selects after, so that a lane has all of them in flight at once and the wave never diverges)
    const float *a = aov + m * 8;
    const float A0 = albedo_floor(a[0]), A1 = albedo_floor(a[1]), A2 = albedo_floor(a[2]);
    const float c0 = color[m * 3], c1 = color[m * 3 + 1], c2 = color[m * 3 + 2];
    const float v = out_variance ? variance[m] : 0.0f;
    const bool ok = usable(r);
    out_color[m * 3] = ok ? r.e[0] * A0 : c0;
    out_color[m * 3 + 1] = ok ? r.e[1] * A1 : c1;
    out_color[m * 3 + 2] = ok ? r.e[2] * A2 : c2;
    if (!out_variance) return;
    const float la = lum(A0, A1, A2);
    out_variance[m] = ok ? r.v * (la * la) : v;
}

/* Luminance variance of the mean from the moments of n samples (s1, s2: sums of v and v*v per channel, in double):
 *   for c: m = s1[c]/n;  q = s2[c]/n - m*m;  var_c = max(q, 0) * n / (n - 1) / n;  v += (w_c * w_c) * var_c   (v from 0.0, c = 0, 1, 2)
 * rounded once to float (a NaN q stays NaN). */
MCPT_DN float luminance_variance(const double *s1, const double *s2, double n) {
    const double wc[3] = {0.2126, 0.7152, 0.0722};
    double v = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double m = s1[c] / n;
        const double q = s2[c] / n - m * m;
        const double var = (q < 0.0 ? 0.0 : q) * n / (n - 1.0) / n;
        v = v + (wc[c] * wc[c]) * var;
    }
    return (float)v;
}

}  // namespace dn
}  // namespace mcpt

#undef MCPT_DN

#if defined(__HIPCC__) || defined(__HIP__)
#include "mcpt_kernels.h"

namespace mcpt {
// Launchers of csrc/mcpt_denoise.hip (all asynchronous on `st`).
// AOV pass of one chunk of whole pixels [p0, p0 + n / aov_spp): the (pixel, sample) keys of its n rays, pixel-major ...
void launch_aov_keys(uint32_t p0, uint32_t n, int32_t aov_spp, uint32_t *pixel, uint32_t *sample, hipStream_t st);
// ... the per-sample records of the traced rays {albedo.rgb, depth} {normal.xyz, hit} ...
void launch_aov_resolve(const DevScene &S, uint32_t n, const float4 *ray_o, const float4 *ray_d, const uint4 *hit, float4 *s0, float4 *s1, hipStream_t st);
// ... or, following specular chains (mcpt_render_aovs_ex), one step for the n rays of a list whose samples have followed b bounces (chain_in
// {thr.rgb, j as bits} and tsum_in; both nullptr for the camera rays: j = i): a finished sample writes s0[j], s1[j]; a continuing one
// (b < max_b) is appended to next_o / next_d / chain_out / tsum_out at an index counted on *n_next ...
void launch_aov_chain(const DevScene &S, uint32_t n, int32_t b, int32_t max_b, const float4 *ray_o, const float4 *ray_d, const uint4 *hit,
                      const float4 *chain_in, const double *tsum_in, float4 *s0, float4 *s1, float4 *next_o, float4 *next_d, float4 *chain_out,
                      double *tsum_out, uint32_t *n_next, hipStream_t st);
// ... folded in sample order into aov[8 (p0 + i) ...] for the chunk's n_pix pixels
void launch_aov_fold(uint32_t p0, uint32_t n_pix, int32_t aov_spp, const float4 *s0, const float4 *s1, float *aov, hipStream_t st);
// var[m] = dn::luminance_variance of the moments (6 doubles per pixel) of n samples, for every pixel of the frame
void launch_dn_variance(uint32_t n_px, const double *moments, int32_t n, float *var, hipStream_t st);
// var[m] = dn::luminance_variance of the moments of spp_map[m] samples (an adaptive frame's count map); 0 where spp_map[m] is 0
void launch_dn_variance_map(uint32_t n_px, const double *moments, const int32_t *spp_map, float *var, hipStream_t st);
// The whole filter: prep -> o.iterations a-trous passes (rec0 <-> rec1, W*H records each; grad W*H) -> remodulation into out (W*H*3).
void launch_denoise(int W, int H, const dn::Opts &o, const float *color, const float *variance, const float *aov, dn::Rec *rec0, dn::Rec *rec1,
                    float2 *grad, float *out, hipStream_t st);
// The filter with the history a feedback sequence keeps: right after iteration k (1..o.iterations) k_dn_feedback writes dn::feedback_pixel of
// that iteration's records into fb_color (W*H*3) and fb_variance (W*H; nullable).  It only reads the records, so iteration k + 1 follows it
// at once.  k 0: launch_denoise, launch for launch.
void launch_denoise_feedback(int W, int H, const dn::Opts &o, const float *color, const float *variance, const float *aov, dn::Rec *rec0,
                             dn::Rec *rec1, float2 *grad, float *out, int k, float *fb_color, float *fb_variance, hipStream_t st);
}  // namespace mcpt
#endif
#endif  // MCPT_DENOISE_H
