/*
 * mcpt_probe_depth.h -- the rule of probe visibility (include/mcpt.h: mcpt_query_probe_depth, mcpt_probe_shade_visible,
 * mcpt_bake_probe_volume and their host forms): the 8 x 8 octahedral map of distance moments a probe carries, the texel of a vector,
 * the cos^32 fold weight, the back-face test that retires a buried probe, and the occlusion-aware grid lookup.
 *
 * Like csrc/mcpt_sh.h, which it builds on: every function is callable from the host and from the device, both compilations run with
 * -ffp-contract=off, float32 in the written order, and only + - * /, sqrtf, fabsf, fminf, fmaxf and floorf are used.  A three-term dot
 * product is a.x * b.x + (a.y * b.y + a.z * b.z), the order of csrc/mcpt_device.h.  csrc/mcpt_probes.hip holds the kernels and the
 * host loops; tests/test_probe_depth_cpu.py checks the host loops against the numpy restatement of tests/probe_depth_cases.py,
 * tests/test_gpu_probe_depth.py the device against the host loops, bit for bit.
 */
#ifndef MCPT_PROBE_DEPTH_H
#define MCPT_PROBE_DEPTH_H

#include "mcpt_sh.h"

namespace mcpt {
namespace pd {

constexpr int32_t kRes = 8;                        // MCPT_PROBE_DEPTH_RES
constexpr int32_t kTexels = kRes * kRes;           // one wave
constexpr int32_t kRow = kTexels * 3;              // floats per probe: (W, S1, S2) per texel
constexpr int32_t kMaxProbes = 0x7fffffff / kRow;  // 192 n fits a 32-bit index
constexpr float kFltMax = 3.4028234663852886e38f;

MCPT_SH float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
MCPT_SH float sgn(float v) { return v >= 0.f ? 1.0f : -1.0f; }

// The unit direction c_j of texel j = 8 ty + tx: the centre of the texel in the octahedral square [-1, 1]^2, unfolded.
MCPT_SH void texel_dir(int32_t j, float c[3]) {
    const int32_t tx = j & 7, ty = j >> 3;
    const float ox = ((float)tx + 0.5f) * 0.25f - 1.0f, oy = ((float)ty + 0.5f) * 0.25f - 1.0f;
    const float az = (1.0f - fabsf(ox)) - fabsf(oy);
    float x = ox, y = oy;
    if (az < 0.f) {
        x = (1.0f - fabsf(oy)) * sgn(ox);
        y = (1.0f - fabsf(ox)) * sgn(oy);
    }
    const float l = sqrtf((x * x + y * y) + az * az);
    c[0] = x / l;
    c[1] = y / l;
    c[2] = az / l;
}

// The nearest texel of a vector (it need not be unit).  A zero vector, and one whose 1-norm is not finite, have texel 0.
MCPT_SH int32_t texel_of(const float v[3]) {
    const float s = (fabsf(v[0]) + fabsf(v[1])) + fabsf(v[2]);
    if (!(s > 0.f) || !(s <= kFltMax)) return 0;
    float px = v[0] / s, py = v[1] / s;
    if (v[2] < 0.f) {
        const float fx = (1.0f - fabsf(py)) * sgn(px), fy = (1.0f - fabsf(px)) * sgn(py);
        px = fx;
        py = fy;
    }
    int32_t tx = (int32_t)floorf((px + 1.0f) * 4.0f), ty = (int32_t)floorf((py + 1.0f) * 4.0f);
    tx = tx < 0 ? 0 : (tx > 7 ? 7 : tx);
    ty = ty < 0 ? 0 : (ty > 7 ? 7 : ty);
    return 8 * ty + tx;
}

// The weight of a sample of direction d in the texel of direction c: max(dot, 0)^32 by five squarings.
MCPT_SH float fold_weight(const float c[3], const float d[3]) {
    float w = fmaxf(dot3(c, d), 0.f);
    w = w * w;
    w = w * w;
    w = w * w;
    w = w * w;
    w = w * w;
    return w;
}

// One sample folded into a texel's three sums.
MCPT_SH void fold_sample(float w, float r, float &W, float &S1, float &S2) {
    W = W + w;
    S1 = S1 + w * r;
    S2 = S2 + w * (r * r);
}

// A probe is dead when more than backface_max of its samples hit a back face; a probe without samples is alive.
MCPT_SH bool probe_dead(const int32_t *counts, size_t probe, float backface_max) {
    const int32_t n = counts[2 * probe], b = counts[2 * probe + 1];
    return n > 0 && (float)b > backface_max * (float)n;
}

// E / pi at point p for the unit normal n from the grid's coefficients, each corner weighted by trilinear weight x wrap-around
// backface weight x Chebyshev visibility from the corner probe's depth map; *weight (nullable) gets the sum of the weights A.  A == 0
// (every corner dead or invisible): sh::probe_shade's value.
MCPT_SH void shade_visible(const sh::Grid &g, const float *coef, const float *moments, const int32_t *counts, float normal_bias, float backface_max,
                           const float p[3], const float n[3], float out[3], float *weight) {
    int32_t ix, iy, iz;
    float tx, ty, tz;
    sh::grid_axis(p[0], g.origin[0], g.spacing[0], g.dims[0], ix, tx);
    sh::grid_axis(p[1], g.origin[1], g.spacing[1], g.dims[1], iy, ty);
    sh::grid_axis(p[2], g.origin[2], g.spacing[2], g.dims[2], iz, tz);
    const int32_t sx = g.dims[0] > 1 ? 1 : 0, sy = g.dims[1] > 1 ? 1 : 0, sz = g.dims[2] > 1 ? 1 : 0;
    const float q[3] = {p[0] + normal_bias * n[0], p[1] + normal_bias * n[1], p[2] + normal_bias * n[2]};
    size_t base[8];
    float a[8];
    float A = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int32_t c = 0; c < 8; ++c) {
        const int32_t dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        const float wx = dx ? tx : 1.0f - tx, wy = dy ? ty : 1.0f - ty, wz = dz ? tz : 1.0f - tz;
        const float wt = (wz * wy) * wx;
        const int32_t cx = ix + dx * sx, cy = iy + dy * sy, cz = iz + dz * sz;
        const size_t probe = ((size_t)cz * (size_t)g.dims[1] + (size_t)cy) * (size_t)g.dims[0] + (size_t)cx;
        base[c] = probe * (size_t)sh::kRow;
        float P[3];
        sh::grid_point(g, cx, cy, cz, P);
        float ac = 0.f;
        if (!probe_dead(counts, probe, backface_max)) {
            const float u[3] = {P[0] - p[0], P[1] - p[1], P[2] - p[2]};
            const float lu = sqrtf(dot3(u, u));
            const float cosn = lu > 0.f ? dot3(u, n) / lu : 1.0f;
            const float h = (cosn + 1.0f) * 0.5f;
            const float wb = h * h + 0.2f;
            const float v[3] = {q[0] - P[0], q[1] - P[1], q[2] - P[2]};
            const float dist = sqrtf(dot3(v, v));
            const float *m3 = moments + (probe * (size_t)kTexels + (size_t)texel_of(v)) * 3;
            const float W = m3[0], S1 = m3[1], S2 = m3[2];
            float ch = 1.0f;
            if (W > 0.f) {
                const float m = S1 / W, m2 = S2 / W;
                const float var = fabsf(m2 - m * m);
                if (dist > m) {
                    const float dd = dist - m;
                    const float den = var + dd * dd;
                    ch = den > 0.f ? var / den : 0.f;
                    ch = (ch * ch) * ch;
                }
            }
            ac = (wt * wb) * ch;
        }
        a[c] = ac;
        A = A + ac;
    }
    if (weight) *weight = A;
    if (!(A > 0.f)) {
        sh::probe_shade(g, coef, p, n, out);
        return;
    }
    float b[27];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int32_t k = 0; k < 27; ++k) {
        float s = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int32_t c = 0; c < 8; ++c) s = s + a[c] * coef[base[c] + (size_t)k];
        b[k] = s;
    }
    float e[3];
    sh::sh9_irradiance(b, n, e);
    out[0] = e[0] / A;
    out[1] = e[1] / A;
    out[2] = e[2] / A;
}

}  // namespace pd
}  // namespace mcpt

#endif /* MCPT_PROBE_DEPTH_H */
