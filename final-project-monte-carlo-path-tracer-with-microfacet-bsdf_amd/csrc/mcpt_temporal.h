/*
 * mcpt_temporal.h -- the per-sample and per-pixel arithmetic of temporal reuse (include/mcpt.h: mcpt_render_motion, mcpt_temporal_blend).
 *
 * Motion: where the surface point a feature sample hit was on the previous frame's screen.  Blend: the bilinear, depth-validated
 * reprojection of the previous frame's colour and its running average with the new frame.  Accumulate: the blend, and the variance of
 * its result propagated from the variances of its inputs (mcpt_temporal_accumulate, mcpt_sequence_frame).  Every function here is callable from the
 * host and from the device, and both compilations (hipcc -ffp-contract=off for gfx950; g++ -std=c++17 -O2 -ffp-contract=off) give the
 * same bits: float32 arithmetic in a fixed order, no FMA, correctly rounded f32 division and square root, floorf.
 * tests/test_temporal_cpu.py checks the host build against numpy restatements and tests/test_gpu_temporal.py checks the device against
 * the host build bit for bit.  csrc/mcpt_temporal.hip holds the kernels.
 *
 * Per-sample motion record and per-pixel motion record alike: 4 floats {dx, dy, prev_depth, valid}.
 */
#ifndef MCPT_TEMPORAL_H
#define MCPT_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "mcpt_denoise.h"  // dn::lum: the luminance the kMoments flavour takes its moments of

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MCPT_TP static __host__ __device__ __forceinline__
#else
#include <math.h>
#define MCPT_TP static inline
#endif

namespace mcpt {
namespace tp {

constexpr int32_t kMaxHistory = 4096;

// What a projection reads of a camera: scale and aspect exactly those of the camera rays (make_camera, csrc/mcpt_wavefront.hip).
struct Cam {
    int32_t width, height;
    float scale, aspect;
    float eye[3];
    float orient[9];  // row-major, columns = left, up, forward
};

// Options after the defaults of include/mcpt.h have been applied.
struct Opts {
    float max_history;  // 1..4096, an integer value
    float depth_tol;    // > 0
};

// 0 on success, -1 if an option is out of range.
MCPT_TP int resolve_opts(const mcpt_temporal_opts &o, Opts &out) {
    for (int k = 0; k < 6; ++k)
        if (o.reserved[k] != 0) return -1;
    const int32_t mh = o.max_history == 0 ? 32 : o.max_history;
    if (mh < 1 || mh > kMaxHistory) return -1;
    const float dt = o.depth_tol == 0.0f ? 0.02f : o.depth_tol;
    if (!(dt > 0.0f && dt <= 3.0e38f)) return -1;  // (positive and finite; NaN fails)
    out.max_history = (float)mh;
    out.depth_tol = dt;
    return 0;
}

// History rejection after the defaults of include/mcpt.h have been applied (mcpt_history_opts).
constexpr float kDefaultNormalMin = 0.9f;
constexpr float kDefaultClampK = 1.0f;
struct HistOpts {
    int32_t normal_test, color_clamp;  // 0 or 1
    float normal_min;                  // in (0, 1]
    float clamp_k;                     // > 0, finite
};

// 0 on success, -1 if an option is out of range.  Both values are checked whether or not their switch is on.
MCPT_TP int resolve_history_opts(const mcpt_history_opts &o, HistOpts &out) {
    for (int k = 0; k < 4; ++k)
        if (o.reserved[k] != 0) return -1;
    if ((o.normal_test != 0 && o.normal_test != 1) || (o.color_clamp != 0 && o.color_clamp != 1)) return -1;
    const float nm = o.normal_min == 0.0f ? kDefaultNormalMin : o.normal_min;
    if (!(nm > 0.0f && nm <= 1.0f)) return -1;  // (NaN fails)
    const float ck = o.clamp_k == 0.0f ? kDefaultClampK : o.clamp_k;
    if (!(ck > 0.0f && ck <= 3.0e38f)) return -1;  // (positive and finite; NaN fails)
    out.normal_test = o.normal_test;
    out.color_clamp = o.color_clamp;
    out.normal_min = nm;
    out.clamp_k = ck;
    return 0;
}

MCPT_TP bool finite_f(float x) { return x - x == 0.0f; }  // false for +-inf and NaN

/* The screen position of p: q = orient^T (p - eye) in the 3-term dot order x + (y + z); the inverse of the camera ray's x, y
 * (a pinhole through eye: a lens offset is ignored), in pixels with pixel i covering [i, i + 1).  false if q.z <= 0 (or NaN). */
MCPT_TP bool project(const Cam &c, const float p[3], float &sx, float &sy) {
    const float dx = p[0] - c.eye[0], dy = p[1] - c.eye[1], dz = p[2] - c.eye[2];
    const float qx = c.orient[0] * dx + (c.orient[3] * dy + c.orient[6] * dz);
    const float qy = c.orient[1] * dx + (c.orient[4] * dy + c.orient[7] * dz);
    const float qz = c.orient[2] * dx + (c.orient[5] * dy + c.orient[8] * dz);
    if (!(qz > 0.0f)) return false;
    sx = (1.0f - (qx / qz) / (c.aspect * c.scale)) * (0.5f * (float)c.width);
    sy = (1.0f - (qy / qz) / c.scale) * (0.5f * (float)c.height);
    return true;
}

// v0 + (e1 u + e2 v) of a triangle record whose first nine floats are v0, e1, e2 (TriGeom, csrc/mcpt_internal.h)
MCPT_TP void tri_point(const float *g, float u, float v, float p[3]) {
    p[0] = g[0] + (g[3] * u + g[6] * v);
    p[1] = g[1] + (g[4] * u + g[7] * v);
    p[2] = g[2] + (g[5] * u + g[8] * v);
}

/* The motion record of one hit sample: the point is at p_cur now and was at p_prev when the snapshot was taken.
 *   {proj(prev, p_prev) - proj(cur, p_cur), |p_prev - eye_prev|, 1};  {0, 0, 0, 0} if either projection has q.z <= 0. */
MCPT_TP void sample_motion(const Cam &cur, const Cam &prev, const float p_cur[3], const float p_prev[3], float out[4]) {
    float cx, cy, px, py;
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (!project(cur, p_cur, cx, cy) || !project(prev, p_prev, px, py)) return;
    const float dx = p_prev[0] - prev.eye[0], dy = p_prev[1] - prev.eye[1], dz = p_prev[2] - prev.eye[2];
    out[0] = px - cx;
    out[1] = py - cy;
    out[2] = sqrtf(dx * dx + (dy * dy + dz * dz));
    out[3] = 1.0f;
}

/* The samples of a pixel (4 floats each) folded in sample order: dx, dy and prev_depth are sums over the valid samples divided by their
 * number (0 without one); valid = that number / spp. */
MCPT_TP void fold_pixel(const float *s, int32_t spp, float out[4]) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    int32_t n = 0;
    for (int32_t k = 0; k < spp; ++k) {
        if (!(s[4 * k + 3] > 0.0f)) continue;
        a0 = a0 + s[4 * k];
        a1 = a1 + s[4 * k + 1];
        a2 = a2 + s[4 * k + 2];
        ++n;
    }
    const float fn = (float)n;
    out[0] = n > 0 ? a0 / fn : 0.0f;
    out[1] = n > 0 ? a1 / fn : 0.0f;
    out[2] = n > 0 ? a2 / fn : 0.0f;
    out[3] = fn / (float)spp;
}

/* The arrays of a W x H frame the rule reads and writes, as three small sets of pointers.  A member a flavour does not use may be null.
 * This frame's planes: color 3 floats per pixel, variance 1 (its luminance variance of the colour mean), motion 4; the first-hit normal of
 * pixel m at normal[normal_stride m ..] and its first-hit depth at depth[depth_stride m] (stride 3 and 1 for packed arrays, 8 for the
 * channels of an AOV array).  The rule reads the normal only with the normal test and never the depth: the kernel copies both into the
 * next history set (csrc/mcpt_temporal.hip).  The kWeight flavour alone reads the last two: count, the W*H per-pixel sample counts of this
 * frame, or, where count is null, uniform_count for every pixel (s of the rule; s >= 1). */
struct Frame { const float *color, *variance, *motion, *normal; int normal_stride; const float *depth; int depth_stride; const int32_t *count; float uniform_count; };
// The previous history set: color 3 floats per pixel, normal 3 (packed), the others 1.  weight (kWeight only): the samples behind the history.
struct Prev { const float *color, *variance, *depth, *len, *normal, *weight; };
// The next one.  The rule writes color, variance, len and flags (one byte per pixel, nullable), and with kWeight weight; depth and normal
// are the kernel's copies.
struct Next { float *color, *variance, *depth, *len, *normal; uint8_t *flags; float *weight; };
// The moments planes of the kMoments flavour, apart from the sets so that the flavours without it keep their argument layout: the running
// first and second moment of each pixel's luminance, 2 floats per pixel, interleaved and 8-byte aligned; prev is read, next written.
struct Moments { const float *prev; float *next; };

/* What the taps of one pixel's history add up to (steps 2, 3 and the sums of step 5 of the rule in include/mcpt.h). */
struct Taps {
    float sw, s0, s1, s2;  // sum of w, sum of w * colour
    float sv;              // sum of (w * w) * prev.variance (kVar only)
    float nmin;            // the smallest prev.len of the used taps
    bool nskip;            // the normal test skipped a tap that every older test had passed (kNorm only)
    float hmin;            // the smallest prev.weight of the used taps (kWeight only): conservative, as nmin is for len
    float sm1, sm2;        // sum of w * the taps' first and second luminance moment (kMoments only)
};

// The two moments of pixel q: one 8-byte load on the device.
struct Mom2 { float m1, m2; };
MCPT_TP Mom2 load_moments(const float *moments, size_t q) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float2 v = reinterpret_cast<const float2 *>(moments)[q];
    return {v.x, v.y};
#else
    return {moments[q * 2], moments[q * 2 + 1]};
#endif
}
MCPT_TP void store_moments(float *moments, size_t q, float m1, float m2) {
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<float2 *>(moments)[q] = make_float2(m1, m2);
#else
    moments[q * 2] = m1, moments[q * 2 + 1] = m2;
#endif
}

/* The tap loop every flavour shares: the four bilinear taps of pixel (i, j) moved by its motion record, in tap order, with every skip of
 * the rule.  false if no tap is left.  kVar: also sum the taps' variances (p.variance is not read without it).
 * The taps' positions are tested in float before they become indices, so a motion that is huge or not finite reads nothing.
 * kNorm: the normal test of mcpt_temporal_accumulate_ex after the depth test: a tap is skipped if !(d >= normal_min), d the 3-term dot
 * x + (y + z) of p.normal[tap] and this pixel's normal (neither f.normal nor p.normal is read without it).
 * kWeight: a tap is also skipped, together with the prev_len <= 0 test, if !(p.weight[tap] > 0) (a NaN weight skips it), and hmin is the
 * smallest weight of the used taps (p.weight is not read without it).
 * kMoments: also sum w * the taps' luminance moments, over exactly the taps the colour uses (prev_moments is not read without it). */
template <bool kVar, bool kNorm, bool kWeight = false, bool kMoments = false>
MCPT_TP bool gather_taps(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, float normal_min, Taps &t,
                         const float *prev_moments = nullptr) {
    const size_t m = (size_t)j * W + i;
    const float *mv = f.motion + m * 4;
    float n3[3] = {0.0f, 0.0f, 0.0f};
    if (kNorm)
        for (int c = 0; c < 3; ++c) n3[c] = f.normal[m * (size_t)f.normal_stride + c];
    const float fx = (float)i + mv[0], fy = (float)j + mv[1];
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float a = fx - x0, b = fy - y0;
    const float wx[2] = {1.0f - a, a}, wy[2] = {1.0f - b, b};
    const float zp = mv[2], ztol = o.depth_tol * zp;
    float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sv = 0.0f, nmin = 0.0f, hmin = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
    bool any = false, nskip = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const float w = wx[k & 1] * wy[k >> 1];
        const float tx = x0 + (float)(k & 1), ty = y0 + (float)(k >> 1);
        if (w == 0.0f) continue;
        if (!(tx >= 0.0f && tx < (float)W && ty >= 0.0f && ty < (float)H)) continue;
        const size_t q = (size_t)(int)ty * W + (size_t)(int)tx;
        const float n = p.len[q];
        if (n <= 0.0f) continue;
        const float hw = kWeight ? p.weight[q] : 0.0f;
        if (kWeight && !(hw > 0.0f)) continue;
        const float p0 = p.color[q * 3], p1 = p.color[q * 3 + 1], p2 = p.color[q * 3 + 2];
        if (!(finite_f(p0) && finite_f(p1) && finite_f(p2))) continue;
        const float dz = p.depth[q] - zp;
        if (!((dz < 0.0f ? -dz : dz) <= ztol)) continue;  // (a NaN depth on either side rejects the tap)
        if (kNorm) {
            const float d = p.normal[q * 3] * n3[0] + (p.normal[q * 3 + 1] * n3[1] + p.normal[q * 3 + 2] * n3[2]);
            if (!(d >= normal_min)) {  // (a NaN normal on either side rejects the tap)
                nskip = true;
                continue;
            }
        }
        sw = sw + w;
        s0 = s0 + w * p0;
        s1 = s1 + w * p1;
        s2 = s2 + w * p2;
        if (kVar) sv = sv + (w * w) * p.variance[q];
        if (kMoments) {
            const Mom2 mq = load_moments(prev_moments, q);
            sm1 = sm1 + w * mq.m1;
            sm2 = sm2 + w * mq.m2;
        }
        nmin = (!any || n < nmin) ? n : nmin;
        if (kWeight) hmin = (!any || hw < hmin) ? hw : hmin;
        any = true;
    }
    t = {sw, s0, s1, s2, sv, nmin, nskip, hmin, sm1, sm2};
    return any;
}

// The length of a history whose shortest used tap has nmin frames (step 5 of the rule): N = min(nmin + 1, max_history).
MCPT_TP float history_step(float nmin, const Opts &o) {
    const float n1 = nmin + 1.0f;
    return n1 < o.max_history ? n1 : o.max_history;
}

/* One channel of the neighbourhood clamp: the history value h against the mean and deviation of the n finite 3 x 3 neighbours, whose sums
 * s = sum c and s2 = sum c*c were taken from 0 in neighbour order.  max(x, 0) is x > 0 ? x : 0 (a NaN gives 0), and the clamp is two
 * comparisons, t = h < lo ? lo : h;  t > hi ? hi : t, so a bound that is NaN leaves h as it is. */
MCPT_TP float clamp_channel(float h, float s, float s2, float fn, float clamp_k) {
    const float mu = s / fn;
    const float v = s2 / fn - mu * mu;
    const float var = v > 0.0f ? v : 0.0f;
    const float sd = sqrtf(var);
    const float ksd = clamp_k * sd;
    const float lo = mu - ksd, hi = mu + ksd;
    const float t = h < lo ? lo : h;
    return t > hi ? hi : t;
}

/* Step 5 of the kWeight flavour: what a history of weight hmin (> 0) becomes when a frame of s samples joins it.
 *   Hc = min(hmin, (max_history - 1) * s);   Neff = (Hc + s) / s;   the blend's k is 1.f / Neff;   the new weight is Hc + s.
 * k is formed as 1.f / Neff and not as s / (Hc + s) on purpose: with uniform counts, history weights equal to prev_len * s and
 * max_history * s < 2^24 every term is an integer below 2^24, so Neff is the integer N of history_step exactly and the flavour gives the
 * unweighted rule's bits. */
struct WeightStep {
    float neff, weight;
};
MCPT_TP WeightStep weight_step(float hmin, float s, const Opts &o) {
    const float cap = (o.max_history - 1.0f) * s;
    const float hc = hmin < cap ? hmin : cap;
    const float sum = hc + s;
    return {sum / s, sum};
}

// What the rule gives one pixel.  flags: bit 0 the normal test skipped a tap, bit 1 the clamp moved the history.  weight: kWeight only.
// mu1, mu2: kMoments only.
struct Pixel {
    float c0, c1, c2, variance, len;
    uint8_t flags;
    float weight;
    float mu1, mu2;
};

/* The rule at pixel (i, j) of a W x H frame (include/mcpt.h: mcpt_temporal_blend, mcpt_temporal_accumulate[_ex]), once, with compile-time
 * switches; every entry point and kernel is one of its flavours.  Without a switch it is the blend: the bilinear, depth-validated
 * reprojection of the previous colour and its running average with the new one; neither variance is read and Pixel::variance is 0.
 *   kVar   also the variance of the result, from f.variance[m] = v_c, this frame's, and p.variance, the previous result's.  Where the
 *          pixel takes no history it is v_c; otherwise, over the taps the colour used, in tap order and from 0,
 *              sv = sv + (w*w) * p.variance[q];  hv = sv / (sw*sw);  k = 1.f / N;  omk = 1.f - k;  variance = (omk*omk)*hv + (k*k)*v_c:
 *          the variance of hist + (color - hist)*k for independent terms, so a static pixel carries (sum of its frames' variances) / N^2
 *          after N frames.  An hv that is not finite or is negative (a tap's stored variance was) gives v_c: one frame's variance
 *          over-estimates, so a filter guided by it smooths more, never less.  A NaN v_c propagates.  Taps and output pixels are treated as
 *          independent: the covariance bilinear resampling gives neighbours (two outputs that share a tap share its noise) is ignored.
 *   kNorm  the normal test on every tap (gather_taps); flag bit 0.
 *   kClamp the history mean clamped to the 3 x 3 neighbourhood of the new frame, neighbours in dy-then-dx order; a pixel whose history
 *          moved gets flag bit 1 and keeps v_c.
 *   kWeight the history weighted by sample counts (mcpt_temporal_accumulate_weighted): s = (float)f.count[m], or f.uniform_count where
 *          f.count is null (s >= 1); the weight skip and hmin of gather_taps; and in step 5 k = 1.f / Neff, weight = Hc + s (weight_step)
 *          in place of k = 1.f / N.  len stays history_step(nmin): it still counts frames; flags, the normal test, the clamp and the
 *          formula of the variance are untouched.  A pixel that takes no history gets weight s.  For one pixel the per-sample variance
 *          is the same from frame to frame, so counts are the inverse-variance weights up to a factor.  WITH UNIFORM COUNTS, HISTORY
 *          WEIGHTS EQUAL TO prev_len * s AND max_history * s < 2^24 THE FLAVOUR GIVES THE COLOUR, VARIANCE, len AND FLAGS OF THE
 *          UNWEIGHTED RULE BIT FOR BIT, AND weight = len * s (weight_step says why).
 *   kMoments the running first and second moment of the pixel's luminance (mcpt_temporal_accumulate_moments; used without kVar: this flavour
 *          reads and writes no variance plane, csrc/mcpt_moments.h derives the variance from the moments).  l = dn::lum(colour) of the new
 *          frame, m1 = l, m2 = l*l.  Where the pixel takes history, over the taps the colour used, in tap order and from 0,
 *              sm1 = sm1 + w * mo.prev[tap].m1;  hm1 = sm1 / sw;  mu1 = hm1 + (m1 - hm1) * k    (likewise mu2), k the colour's own.
 *          An hm1 or hm2 that is not finite (a tap's stored moment was not) restarts both: (mu1, mu2) = (m1, m2), as for a pixel that
 *          takes no history.  The clamp moves the colour history only, never the moments.  Colour, len and flags are untouched.
 * A pixel that takes no history (motion.valid <= 0, a colour that is not finite, no tap left) gets its own colour, v_c, length 1, flags 0. */
template <bool kVar, bool kNorm, bool kClamp, bool kWeight = false, bool kMoments = false>
MCPT_TP Pixel reuse_pixel(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, const HistOpts &ho, const Moments &mo = Moments{}) {
    const size_t m = (size_t)j * W + i;
    const float c0 = f.color[m * 3], c1 = f.color[m * 3 + 1], c2 = f.color[m * 3 + 2];
    const float vc = kVar ? f.variance[m] : 0.0f;
    const float s = kWeight ? (f.count ? (float)f.count[m] : f.uniform_count) : 0.0f;
    const float l = kMoments ? dn::lum(c0, c1, c2) : 0.0f;
    const float m1 = l, m2 = l * l;
    Pixel r = {c0, c1, c2, vc, 1.0f, 0, s, m1, m2};
    Taps t;
    if (f.motion[m * 4 + 3] > 0.0f && finite_f(c0) && finite_f(c1) && finite_f(c2) &&
        gather_taps<kVar, kNorm, kWeight, kMoments>(W, H, i, j, f, p, o, ho.normal_min, t, mo.prev)) {
        float h0 = t.s0 / t.sw, h1 = t.s1 / t.sw, h2 = t.s2 / t.sw;
        bool clamped = false;
        if (kNorm && t.nskip) r.flags |= 1;
        if (kClamp) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = i + dx, y = j + dy;
                    if (x < 0 || x >= W || y < 0 || y >= H) continue;
                    const size_t q = (size_t)y * W + x;
                    const float q0 = f.color[q * 3], q1 = f.color[q * 3 + 1], q2 = f.color[q * 3 + 2];
                    if (!(finite_f(q0) && finite_f(q1) && finite_f(q2))) continue;
                    a0 = a0 + q0;
                    a1 = a1 + q1;
                    a2 = a2 + q2;
                    b0 = b0 + q0 * q0;
                    b1 = b1 + q1 * q1;
                    b2 = b2 + q2 * q2;
                    ++n;
                }
            const float fn = (float)n;  // (n >= 1: the pixel itself is finite)
            const float a[3] = {a0, a1, a2}, b[3] = {b0, b1, b2};
            float g[3] = {h0, h1, h2};
            for (int c = 0; c < 3; ++c) g[c] = clamp_channel(g[c], a[c], b[c], fn, ho.clamp_k);
            clamped = g[0] != h0 || g[1] != h1 || g[2] != h2;
            h0 = g[0], h1 = g[1], h2 = g[2];
            if (clamped) r.flags |= 2;
        }
        const float N = history_step(t.nmin, o);
        float k = 1.0f / N;
        if (kWeight) {
            const WeightStep ws = weight_step(t.hmin, s, o);
            k = 1.0f / ws.neff;
            r.weight = ws.weight;
        }
        r.c0 = h0 + (c0 - h0) * k;
        r.c1 = h1 + (c1 - h1) * k;
        r.c2 = h2 + (c2 - h2) * k;
        r.len = N;
        if (kVar) {
            const float hv = t.sv / (t.sw * t.sw);
            const float omk = 1.0f - k;
            if (!clamped && finite_f(hv) && hv >= 0.0f) r.variance = (omk * omk) * hv + (k * k) * vc;
        }
        if (kMoments) {
            const float hm1 = t.sm1 / t.sw, hm2 = t.sm2 / t.sw;
            if (finite_f(hm1) && finite_f(hm2)) {
                r.mu1 = hm1 + (m1 - hm1) * k;
                r.mu2 = hm2 + (m2 - hm2) * k;
            }
        }
    }
    return r;
}

// The pixel's results into the next set: n.color[3 m ..], n.len[m]; with kVar n.variance[m]; with kFlags n.flags[m] where given; with
// kWeight n.weight[m]; with kMoments next_moments[2 m ..].
template <bool kVar, bool kFlags, bool kWeight = false, bool kMoments = false>
MCPT_TP void store_pixel(const Next &n, size_t m, const Pixel &r, float *next_moments = nullptr) {
    n.color[m * 3] = r.c0;
    n.color[m * 3 + 1] = r.c1;
    n.color[m * 3 + 2] = r.c2;
    if (kVar) n.variance[m] = r.variance;
    n.len[m] = r.len;
    if (kFlags && n.flags) n.flags[m] = r.flags;
    if (kWeight) n.weight[m] = r.weight;
    if (kMoments) store_moments(next_moments, m, r.mu1, r.mu2);
}

// The blend at pixel (i, j) (mcpt_temporal_blend), stored.
MCPT_TP void blend_pixel(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, const Next &n) {
    store_pixel<false, false>(n, (size_t)j * W + i, reuse_pixel<false, false, false>(W, H, i, j, f, p, o, HistOpts{}));
}

/* The accumulation with history rejection at pixel (i, j) (mcpt_temporal_accumulate_ex), stored: the flavour ho's switches select.  With
 * ho.normal_test 0 neither normal array is read; with both switches 0 this is mcpt_temporal_accumulate's rule (flags 0). */
MCPT_TP void accumulate_pixel_ex(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, const HistOpts &ho, const Next &n) {
    const Pixel r = ho.normal_test ? (ho.color_clamp ? reuse_pixel<true, true, true>(W, H, i, j, f, p, o, ho) : reuse_pixel<true, true, false>(W, H, i, j, f, p, o, ho))
                                   : (ho.color_clamp ? reuse_pixel<true, false, true>(W, H, i, j, f, p, o, ho) : reuse_pixel<true, false, false>(W, H, i, j, f, p, o, ho));
    store_pixel<true, true>(n, (size_t)j * W + i, r);
}

/* The weighted accumulation at pixel (i, j) (mcpt_temporal_accumulate_weighted), stored: accumulate_pixel_ex's flavours with kWeight. */
MCPT_TP void accumulate_pixel_weighted(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, const HistOpts &ho, const Next &n) {
    const Pixel r = ho.normal_test ? (ho.color_clamp ? reuse_pixel<true, true, true, true>(W, H, i, j, f, p, o, ho) : reuse_pixel<true, true, false, true>(W, H, i, j, f, p, o, ho))
                                   : (ho.color_clamp ? reuse_pixel<true, false, true, true>(W, H, i, j, f, p, o, ho) : reuse_pixel<true, false, false, true>(W, H, i, j, f, p, o, ho));
    store_pixel<true, true, true>(n, (size_t)j * W + i, r);
}

/* The accumulation of colour and luminance moments at pixel (i, j) (mcpt_temporal_accumulate_moments), stored: accumulate_pixel_ex's
 * flavours with kMoments in place of kVar.  Neither variance plane is touched. */
MCPT_TP void accumulate_pixel_moments(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, const HistOpts &ho, const Next &n,
                                      const Moments &mo) {
    const Pixel r = ho.normal_test ? (ho.color_clamp ? reuse_pixel<false, true, true, false, true>(W, H, i, j, f, p, o, ho, mo) : reuse_pixel<false, true, false, false, true>(W, H, i, j, f, p, o, ho, mo))
                                   : (ho.color_clamp ? reuse_pixel<false, false, true, false, true>(W, H, i, j, f, p, o, ho, mo) : reuse_pixel<false, false, false, false, true>(W, H, i, j, f, p, o, ho, mo));
    store_pixel<false, true, false, true>(n, (size_t)j * W + i, r, mo.next);
}

/* The history length pixel (i, j) is about to get (include/mcpt.h: mcpt_temporal_history_len): steps 1-4 of the rule and the N of step 5,
 * with the new colour taken to be finite.  motion.valid <= 0, or no tap left: 1; otherwise history_step.  The taps and their skips are
 * gather_taps<false, kNorm>'s, the normal test included when ho.normal_test is 1; the colour clamp does not enter, because a clamped
 * history keeps its length.  So the value equals the length accumulate_pixel / accumulate_pixel_ex give on the same inputs for every pixel
 * whose new colour is finite, and it is known before the frame is rendered: neither f.color nor f.variance is read. */
MCPT_TP float history_len_pixel(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, const HistOpts &ho) {
    if (!(f.motion[((size_t)j * W + i) * 4 + 3] > 0.0f)) return 1.0f;
    Taps t;
    const bool any = ho.normal_test ? gather_taps<false, true>(W, H, i, j, f, p, o, ho.normal_min, t) : gather_taps<false, false>(W, H, i, j, f, p, o, ho.normal_min, t);
    return any ? history_step(t.nmin, o) : 1.0f;
}

/* The history weight pixel (i, j) is about to get (include/mcpt.h: mcpt_temporal_history_weight), the analogue of history_len_pixel: steps
 * 1-4 of the kWeight flavour -- the weight skip, and the normal test when ho.normal_test is 1 -- and the hmin of its taps; 0 where the pixel
 * takes no history (motion.valid <= 0, no tap left).  Neither colour nor variance is read.  So for every pixel whose new colour is finite
 * the accumulation's weight equals min(this, (max_history - 1) * s) + s. */
MCPT_TP float history_weight_pixel(int W, int H, int i, int j, const Frame &f, const Prev &p, const Opts &o, const HistOpts &ho) {
    if (!(f.motion[((size_t)j * W + i) * 4 + 3] > 0.0f)) return 0.0f;
    Taps t;
    const bool any = ho.normal_test ? gather_taps<false, true, true>(W, H, i, j, f, p, o, ho.normal_min, t) : gather_taps<false, false, true>(W, H, i, j, f, p, o, ho.normal_min, t);
    return any ? t.hmin : 0.0f;
}

/* The Neff the weighted blend will use for a pixel whose history has weight H if the pixel stops at n samples (weight_step with s = n),
 * the guide of mcpt_render_adaptive_weighted; 1 if !(H > 0) (no history, or a NaN).  It is >= 1 and does not increase when n doubles. */
MCPT_TP float weight_guide(float H, int32_t n, float max_history) {
    if (!(H > 0.0f)) return 1.0f;
    const Opts o = {max_history, 0.0f};
    return weight_step(H, (float)n, o).neff;
}

/* The same four on plain packed arrays, for callers without the structs (the CPU builds of tests/native): color, prev_color 3 floats per
 * pixel; motion 4; normal at normal[normal_stride m ..], prev_normal packed, both read only with ho.normal_test; out_flags nullable. */
MCPT_TP void blend_pixel(int W, int H, int i, int j, const float *color, const float *motion, const float *prev_color, const float *prev_depth,
                         const float *prev_len, const Opts &o, float *out_color, float *out_len) {
    blend_pixel(W, H, i, j, Frame{color, nullptr, motion, nullptr, 3, nullptr, 1}, Prev{prev_color, nullptr, prev_depth, prev_len, nullptr}, o,
                Next{out_color, nullptr, nullptr, out_len, nullptr, nullptr});
}
MCPT_TP void accumulate_pixel_ex(int W, int H, int i, int j, const float *color, const float *variance, const float *motion, const float *normal,
                                 int normal_stride, const float *prev_color, const float *prev_variance, const float *prev_depth, const float *prev_len,
                                 const float *prev_normal, const Opts &o, const HistOpts &ho, float *out_color, float *out_variance, float *out_len,
                                 uint8_t *out_flags) {
    accumulate_pixel_ex(W, H, i, j, Frame{color, variance, motion, normal, normal_stride, nullptr, 1},
                        Prev{prev_color, prev_variance, prev_depth, prev_len, prev_normal}, o, ho,
                        Next{out_color, out_variance, nullptr, out_len, nullptr, out_flags});
}
MCPT_TP void accumulate_pixel(int W, int H, int i, int j, const float *color, const float *variance, const float *motion, const float *prev_color,
                              const float *prev_variance, const float *prev_depth, const float *prev_len, const Opts &o, float *out_color,
                              float *out_variance, float *out_len) {
    accumulate_pixel_ex(W, H, i, j, color, variance, motion, nullptr, 3, prev_color, prev_variance, prev_depth, prev_len, nullptr, o, HistOpts{}, out_color,
                        out_variance, out_len, nullptr);
}
MCPT_TP float history_len_pixel(int W, int H, int i, int j, const float *motion, const float *normal, int normal_stride, const float *prev_color,
                                const float *prev_depth, const float *prev_len, const float *prev_normal, const Opts &o, const HistOpts &ho) {
    return history_len_pixel(W, H, i, j, Frame{nullptr, nullptr, motion, normal, normal_stride, nullptr, 1},
                             Prev{prev_color, nullptr, prev_depth, prev_len, prev_normal}, o, ho);
}

// count nullable (W*H int32): uniform_count for every pixel then
MCPT_TP void accumulate_pixel_weighted(int W, int H, int i, int j, const float *color, const float *variance, const float *motion, const float *normal,
                                       int normal_stride, const int32_t *count, float uniform_count, const float *prev_color, const float *prev_variance,
                                       const float *prev_depth, const float *prev_len, const float *prev_normal, const float *prev_weight, const Opts &o,
                                       const HistOpts &ho, float *out_color, float *out_variance, float *out_len, uint8_t *out_flags, float *out_weight) {
    accumulate_pixel_weighted(W, H, i, j, Frame{color, variance, motion, normal, normal_stride, nullptr, 1, count, uniform_count},
                              Prev{prev_color, prev_variance, prev_depth, prev_len, prev_normal, prev_weight}, o, ho,
                              Next{out_color, out_variance, nullptr, out_len, nullptr, out_flags, out_weight});
}
MCPT_TP void accumulate_pixel_moments(int W, int H, int i, int j, const float *color, const float *motion, const float *normal, int normal_stride,
                                      const float *prev_color, const float *prev_depth, const float *prev_len, const float *prev_normal,
                                      const float *prev_moments, const Opts &o, const HistOpts &ho, float *out_color, float *out_len, uint8_t *out_flags,
                                      float *out_moments) {
    accumulate_pixel_moments(W, H, i, j, Frame{color, nullptr, motion, normal, normal_stride, nullptr, 1},
                             Prev{prev_color, nullptr, prev_depth, prev_len, prev_normal}, o, ho,
                             Next{out_color, nullptr, nullptr, out_len, nullptr, out_flags}, Moments{prev_moments, out_moments});
}
MCPT_TP float history_weight_pixel(int W, int H, int i, int j, const float *motion, const float *normal, int normal_stride, const float *prev_color,
                                   const float *prev_depth, const float *prev_len, const float *prev_normal, const float *prev_weight, const Opts &o,
                                   const HistOpts &ho) {
    return history_weight_pixel(W, H, i, j, Frame{nullptr, nullptr, motion, normal, normal_stride, nullptr, 1},
                                Prev{prev_color, nullptr, prev_depth, prev_len, prev_normal, prev_weight}, o, ho);
}

/* The stopping threshold of a guided adaptive pixel (include/mcpt.h: mcpt_render_adaptive_guided): threshold * sqrt(g) in double, with
 * g = guide if guide >= 1 and 1 otherwise, so that a NaN, zero or negative guide leaves the plain rule (sqrt(1.0) is exactly 1). */
MCPT_TP double guided_threshold(double threshold, float guide) {
    const double g = guide >= 1.0f ? (double)guide : 1.0;
    return threshold * sqrt(g);
}

}  // namespace tp
}  // namespace mcpt

#include "mcpt_specular_motion.h"  // the motion of a sample seen through a mirror / glass chain (mcpt_render_motion_ex)

#undef MCPT_TP

#if defined(__HIPCC__) || defined(__HIP__)
#include "mcpt_kernels.h"

namespace mcpt {
// Launchers of csrc/mcpt_temporal.hip (all asynchronous on `st`).
// The motion records of the n traced camera rays of a chunk of the AOV pass (csrc/mcpt_denoise.hip): prev_tri / prev_sph are the
// snapshot's TriGeom and SphereRec arrays (the live ones for a scene without a snapshot) ...
void launch_motion_resolve(const DevScene &S, const TriGeom *prev_tri, const SphereRec *prev_sph, const tp::Cam &cur, const tp::Cam &prev, uint32_t n,
                           const float4 *ray_o, const float4 *ray_d, const uint4 *hit, float4 *rec, hipStream_t st);
// One step of the specular chains (mcpt_render_motion_ex; k_motion_chain): list entry i is ray (ray_o, ray_d)[i] with its hit and, after the
// first step, chain_in[i] = {reflections so far, -, -, sample j}; a sample that stops writes rec[j], one that goes on is appended to
// (next_o, next_d, chain_out) at a position counted in *n_next.  maps: six planes of map_stride float4, entry j of each the sample's.
void launch_motion_chain(const DevScene &S, const TriGeom *prev_tri, const SphereRec *prev_sph, const tp::Cam &cur, const tp::Cam &prev, uint32_t n, int32_t b,
                         int32_t max_b, const float4 *ray_o, const float4 *ray_d, const uint4 *hit, const float4 *chain_in, float4 *rec, float4 *maps,
                         size_t map_stride, float4 *next_o, float4 *next_d, float4 *chain_out, uint32_t *n_next, hipStream_t st);
// ... folded in sample order into motion[4 (p0 + i) ...] for the chunk's n_pix pixels
void launch_motion_fold(uint32_t p0, uint32_t n_pix, int32_t spp, const float4 *rec, float *motion, hipStream_t st);
// The rule over a W x H frame, 16 x 16 pixels per block (tp::Frame, tp::Prev and tp::Next say what each flavour reads and writes).
// The blend (k_temporal_blend)
void launch_temporal_blend(int W, int H, const tp::Opts &o, const tp::Frame &f, const tp::Prev &p, const tp::Next &n, hipStream_t st);
// The accumulation (k_temporal_accumulate<kNorm, kClamp>, the instantiation ho's switches select; both 0: mcpt_temporal_accumulate's).  It
// also leaves the next history set complete: f.depth != nullptr: n.depth[m] = the frame's first-hit depth; with ho.normal_test and n.normal
// != nullptr: n.normal[3 m ..] = the frame's first-hit normal.  n.flags is written with a switch on only (with both 0 every flag is 0, and
// the plain instantiation has no store for it).  n.weight != nullptr: the kWeight instantiations (f.count or f.uniform_count, p.weight),
// which also store n.weight[m]; otherwise the instantiations there have always been.
void launch_temporal_accumulate(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, const tp::Next &n,
                                hipStream_t st);
// The accumulation of colour and luminance moments (k_temporal_accumulate<kNorm, kClamp, false, true>): as above without n.weight; reads
// mo.prev, stores mo.next[2 m ..] and touches no variance plane.
void launch_temporal_accumulate_moments(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, const tp::Next &n,
                                        const tp::Moments &mo, hipStream_t st);
// The history length every pixel is about to get (k_history_len: tp::history_len_pixel) into len[m]
void launch_history_len(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, float *len, hipStream_t st);
// The history weight every pixel is about to get (k_history_weight: tp::history_weight_pixel) into weight[m]
void launch_history_weight(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, float *weight, hipStream_t st);
}  // namespace mcpt
#endif
#endif  // MCPT_TEMPORAL_H
