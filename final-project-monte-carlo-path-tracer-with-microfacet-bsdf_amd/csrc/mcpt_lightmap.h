/*
 * mcpt_lightmap.h -- the rule of lightmap baking (include/mcpt.h: mcpt_lightmap_texels, mcpt_lightmap_scatter, mcpt_bake_lightmap and
 * their host forms): which texels of a W x H map a triangle's UV chart covers, the sensor of a covered texel, and the dilation that
 * fills the texels next to a chart.
 *
 * Every function here is callable from the host and from the device, and both compilations run with -ffp-contract=off: the coverage is
 * float64 arithmetic in a fixed order (no FMA, IEEE division), the sensor point and the dilation are float32 arithmetic in a fixed order.
 * csrc/mcpt_lightmap.hip holds the kernels and the host loops; both call these functions and nothing else decides a texel.
 * tests/test_lightmap_cpu.py checks the host loops against a numpy restatement of include/mcpt.h's text, tests/test_gpu_lightmap.py the
 * device against the host loops, bit for bit.
 */
#ifndef MCPT_LIGHTMAP_H
#define MCPT_LIGHTMAP_H

#include "mcpt_internal.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MCPT_LM static __host__ __device__ __forceinline__
#else
#include <math.h>
#define MCPT_LM static inline
#endif

namespace mcpt {
namespace lm {

constexpr int32_t kTile = 8;             // the rasteriser works on 8 x 8-texel tiles: one wave, one lane per texel
constexpr int32_t kNoOwner = 0x7fffffff;  // owner plane: no triangle covers the texel
constexpr int32_t kMaxTexels = 0x7fffffff / 3;

MCPT_LM bool finite_d(double v) { return v - v == 0.0; }  // (false for NaN and the infinities)

// Twice the signed area of the chart triangle in UV space; float inputs widened first.
MCPT_LM double area2(const TriShade &s) {
    const double ax = (double)s.t0[0], ay = (double)s.t0[1], bx = (double)s.t1[0], by = (double)s.t1[1], cx = (double)s.t2[0], cy = (double)s.t2[1];
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// Does the triangle cover the centre of texel (x, y) of a W x H map?  w1, w2: the barycentrics of b = t1 and c = t2 (w0 = 1 - w1 - w2).
// A triangle whose area2 is zero or not finite covers nothing; a NaN weight fails every comparison.  The division by area2 removes the
// chart's winding.
MCPT_LM bool cover(const TriShade &s, int32_t x, int32_t y, int32_t W, int32_t H, double &w1, double &w2) {
    const double ax = (double)s.t0[0], ay = (double)s.t0[1], bx = (double)s.t1[0], by = (double)s.t1[1], cx = (double)s.t2[0], cy = (double)s.t2[1];
    const double px = ((double)x + 0.5) / (double)W, py = ((double)y + 0.5) / (double)H;
    const double a2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    w1 = 0.0;
    w2 = 0.0;
    if (a2 == 0.0 || !finite_d(a2)) return false;
    w1 = ((px - ax) * (cy - ay) - (py - ay) * (cx - ax)) / a2;
    w2 = ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) / a2;
    const double w0 = 1.0 - w1 - w2;
    return w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0;
}

// The point of barycentrics (u, v) on the live record: the expression of k_query_resolve (csrc/mcpt_rayquery.hip).
MCPT_LM void point(const TriGeom &g, float u, float v, float p[3]) {
    p[0] = g.v0[0] + (g.e1x * u + g.e2xy[0] * v);
    p[1] = g.v0[1] + (g.e1yz[0] * u + g.e2xy[1] * v);
    p[2] = g.v0[2] + (g.e1yz[1] * u + g.e2z * v);
}

// The tiles a triangle's chart can cover: tiles [tx0, tx0 + ntx) x [ty0, ty0 + nty) of the map, nothing when ntx == 0.  An optimisation
// only: it must contain every texel cover() accepts.  A covered centre lies in the chart's bounding box up to the rounding of cover(),
// which is a few units of 2^-53 of the coordinates' magnitude; the box is widened by a whole texel on every side, and charts whose
// coordinates are so large (>= 2^20) that this rounding could approach a texel of the largest map get the whole map.  Not finite: nothing.
MCPT_LM void tile_box(const TriShade &s, int32_t W, int32_t H, int32_t &tx0, int32_t &ty0, int32_t &ntx, int32_t &nty) {
    tx0 = ty0 = ntx = nty = 0;
    const double u[3] = {(double)s.t0[0], (double)s.t1[0], (double)s.t2[0]}, v[3] = {(double)s.t0[1], (double)s.t1[1], (double)s.t2[1]};
    const double a2 = area2(s);
    if (a2 == 0.0 || !finite_d(a2)) return;  // (covers nothing; a non-finite coordinate makes a2 non-finite or is caught below)
    double ulo = u[0], uhi = u[0], vlo = v[0], vhi = v[0];
    for (int k = 1; k < 3; ++k) {
        ulo = u[k] < ulo ? u[k] : ulo;
        uhi = u[k] > uhi ? u[k] : uhi;
        vlo = v[k] < vlo ? v[k] : vlo;
        vhi = v[k] > vhi ? v[k] : vhi;
    }
    if (!finite_d(ulo) || !finite_d(uhi) || !finite_d(vlo) || !finite_d(vhi)) return;
    const double big = 1048576.0;
    double x0 = 0.0, x1 = (double)(W - 1), y0 = 0.0, y1 = (double)(H - 1);
    if (ulo > -big && uhi < big && vlo > -big && vhi < big) {
        // centre (x + 0.5) / W in [ulo, uhi]  <=>  x in [ulo * W - 0.5, uhi * W - 0.5]; one texel wider on either side
        const double fx0 = floor(ulo * (double)W - 0.5) - 1.0, fx1 = ceil(uhi * (double)W - 0.5) + 1.0;
        const double fy0 = floor(vlo * (double)H - 0.5) - 1.0, fy1 = ceil(vhi * (double)H - 0.5) + 1.0;
        x0 = fx0 > x0 ? fx0 : x0;
        x1 = fx1 < x1 ? fx1 : x1;
        y0 = fy0 > y0 ? fy0 : y0;
        y1 = fy1 < y1 ? fy1 : y1;
    }
    if (x0 > x1 || y0 > y1) return;  // the chart lies off the map
    tx0 = (int32_t)x0 / kTile;
    ty0 = (int32_t)y0 / kTile;
    ntx = (int32_t)x1 / kTile - tx0 + 1;
    nty = (int32_t)y1 / kTile - ty0 + 1;
}

// One texel of one dilation round.  img / cov: the planes at the start of the round.  A covered texel keeps its value and coverage; an
// uncovered one with n >= 1 neighbours of coverage != 0 takes, per channel, the float sum of their values in the order (-1,-1), (0,-1),
// (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1), starting from 0, divided by (float)n, and coverage 2; one without keeps 0 and coverage 0.
MCPT_LM void dilate_texel(int32_t W, int32_t H, int32_t x, int32_t y, const float *img, const uint8_t *cov, float out[3], uint8_t &cov_out) {
    const size_t t = (size_t)y * (size_t)W + (size_t)x;
    out[0] = img[3 * t];
    out[1] = img[3 * t + 1];
    out[2] = img[3 * t + 2];
    cov_out = cov[t];
    if (cov_out != 0) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    int32_t n = 0;
    for (int32_t dy = -1; dy <= 1; ++dy)
        for (int32_t dx = -1; dx <= 1; ++dx) {
            const int32_t xx = x + dx, yy = y + dy;
            if ((dx == 0 && dy == 0) || xx < 0 || yy < 0 || xx >= W || yy >= H) continue;
            const size_t q = (size_t)yy * (size_t)W + (size_t)xx;
            if (cov[q] == 0) continue;
            s0 = s0 + img[3 * q];
            s1 = s1 + img[3 * q + 1];
            s2 = s2 + img[3 * q + 2];
            ++n;
        }
    if (n == 0) return;
    const float fn = (float)n;
    out[0] = s0 / fn;
    out[1] = s1 / fn;
    out[2] = s2 / fn;
    cov_out = 2;
}

}  // namespace lm
}  // namespace mcpt

#endif /* MCPT_LIGHTMAP_H */
