/*
 * mcpt_sh.h -- the rule of light probes (include/mcpt.h: mcpt_query_probes, mcpt_probe_shade, mcpt_bake_probe_grid and their host
 * forms): the nine real spherical harmonics of order <= 2, the irradiance of a normal from 27 coefficients, and the trilinear lookup in a
 * regular grid of probes.
 *
 * Every function here is callable from the host and from the device, and both compilations run with -ffp-contract=off: float32
 * arithmetic in the written order, no FMA.  csrc/mcpt_probes.hip holds the kernels and the host loops; both call these functions and
 * nothing else decides a value.  tests/test_probes_cpu.py checks the host loops against a numpy restatement of include/mcpt.h's text,
 * tests/test_gpu_probes.py the device against the host loops, bit for bit.
 */
#ifndef MCPT_SH_H
#define MCPT_SH_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MCPT_SH static __host__ __device__ __forceinline__
#else
#include <math.h>
#define MCPT_SH static inline
#endif

namespace mcpt {
namespace sh {

constexpr int32_t kCoef = 9;                      // basis functions
constexpr int32_t kRow = 27;                      // floats per probe: [3j + c], coefficient j of channel c
constexpr int32_t kMaxProbes = 0x7fffffff / 27;   // 27 n fits a 32-bit lane index

// The float roundings of sqrt(1/(4 pi)), sqrt(3/(4 pi)), sqrt(15/(4 pi)), sqrt(5/(16 pi)), sqrt(15/(16 pi)).
constexpr float kY0 = 0.28209479177387814f;
constexpr float kY1 = 0.4886025119029199f;
constexpr float kY2 = 1.0925484305920792f;
constexpr float kY20 = 0.31539156525252005f;
constexpr float kY22 = 0.5462742152960396f;
constexpr float kFourPi = 12.566370614359172f;    // (float)(4 pi): the reciprocal of the uniform-sphere pdf
// The clamped-cosine convolution divided by pi, per band: pi, 2 pi / 3, pi / 4 over pi.
constexpr float kA0 = 1.0f;
constexpr float kA1 = 0.6666666666666666f;
constexpr float kA2 = 0.25f;

// Y_j of the unit direction d = (x, y, z); a product a * b * c is (a * b) * c.
MCPT_SH void sh9_basis(const float d[3], float Y[9]) {
    const float x = d[0], y = d[1], z = d[2];
    Y[0] = kY0;
    Y[1] = kY1 * y;
    Y[2] = kY1 * z;
    Y[3] = kY1 * x;
    Y[4] = kY2 * x * y;
    Y[5] = kY2 * y * z;
    Y[6] = kY20 * (3.0f * z * z - 1.0f);
    Y[7] = kY2 * x * z;
    Y[8] = kY22 * (x * x - y * y);
}

MCPT_SH float band_weight(int32_t j) { return j == 0 ? kA0 : (j < 4 ? kA1 : kA2); }

// E / pi for the unit normal n from the coefficients L[3j + c]: out[c] = sum over j, in index order and starting from 0, of
// (A(j) * L[3j + c]) * Y_j(n).  Not clamped at zero: the ringing of the truncated series can go slightly negative.
MCPT_SH void sh9_irradiance(const float L[27], const float n[3], float out[3]) {
    float Y[9];
    sh9_basis(n, Y);
    float e0 = 0.f, e1 = 0.f, e2 = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int32_t j = 0; j < 9; ++j) {
        const float a = band_weight(j);
        e0 = e0 + (a * L[3 * j]) * Y[j];
        e1 = e1 + (a * L[3 * j + 1]) * Y[j];
        e2 = e2 + (a * L[3 * j + 2]) * Y[j];
    }
    out[0] = e0;
    out[1] = e1;
    out[2] = e2;
}

// A regular grid of probes: probe (ix, iy, iz) sits at origin + (float)i * spacing per axis and has the index (iz * ny + iy) * nx + ix.
struct Grid {
    float origin[3], spacing[3];
    int32_t dims[3];
};

MCPT_SH void grid_point(const Grid &g, int32_t ix, int32_t iy, int32_t iz, float p[3]) {
    p[0] = g.origin[0] + (float)ix * g.spacing[0];
    p[1] = g.origin[1] + (float)iy * g.spacing[1];
    p[2] = g.origin[2] + (float)iz * g.spacing[2];
}

// One axis of the lookup: the cell i0 and the weight t of its upper probe.  g = (p - origin) / spacing clamped to [0, dim - 1] (a NaN
// becomes 0), i0 = min((int)floorf(g), dim - 2), t = g - i0.  dim == 1: i0 = 0, t = 0.
MCPT_SH void grid_axis(float p, float origin, float spacing, int32_t dim, int32_t &i0, float &t) {
    i0 = 0;
    t = 0.f;
    if (dim == 1) return;
    float g = (p - origin) / spacing;
    g = fminf(fmaxf(g, 0.f), (float)(dim - 1));
    const int32_t f = (int32_t)floorf(g);
    i0 = f < dim - 2 ? f : dim - 2;
    t = g - (float)i0;
}

// E / pi at point p for normal n from the grid's coefficients sh[27 * probe + 3j + c]: every coefficient is blended over the eight
// corners of p's cell, b = 0; b = b + w * L_corner for the corners in the order (dz, dy, dx) = 000, 001, 010, 011, 100, 101, 110, 111 with
// w = (wz * wy) * wx, w_axis = 1 - t for d = 0 and t for d = 1; then the sum of sh9_irradiance over the blended coefficients.  Along an
// axis with one probe the upper corner is the probe itself (with weight 0).
MCPT_SH void probe_shade(const Grid &g, const float *sh, const float p[3], const float n[3], float out[3]) {
    int32_t ix, iy, iz;
    float tx, ty, tz;
    grid_axis(p[0], g.origin[0], g.spacing[0], g.dims[0], ix, tx);
    grid_axis(p[1], g.origin[1], g.spacing[1], g.dims[1], iy, ty);
    grid_axis(p[2], g.origin[2], g.spacing[2], g.dims[2], iz, tz);
    const int32_t sx = g.dims[0] > 1 ? 1 : 0, sy = g.dims[1] > 1 ? 1 : 0, sz = g.dims[2] > 1 ? 1 : 0;
    size_t base[8];
    float w[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int32_t c = 0; c < 8; ++c) {
        const int32_t dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        const float wx = dx ? tx : 1.0f - tx, wy = dy ? ty : 1.0f - ty, wz = dz ? tz : 1.0f - tz;
        w[c] = (wz * wy) * wx;
        const size_t probe = ((size_t)(iz + dz * sz) * (size_t)g.dims[1] + (size_t)(iy + dy * sy)) * (size_t)g.dims[0] + (size_t)(ix + dx * sx);
        base[c] = probe * (size_t)kRow;
    }
    float Y[9];
    sh9_basis(n, Y);
    float e[3] = {0.f, 0.f, 0.f};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int32_t j = 0; j < 9; ++j) {
        const float a = band_weight(j);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int32_t ch = 0; ch < 3; ++ch) {
            float b = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int32_t c = 0; c < 8; ++c) b = b + w[c] * sh[base[c] + (size_t)(3 * j + ch)];
            e[ch] = e[ch] + (a * b) * Y[j];
        }
    }
    out[0] = e[0];
    out[1] = e[1];
    out[2] = e[2];
}

}  // namespace sh
}  // namespace mcpt

#endif /* MCPT_SH_H */
