/*
 * mcpt_specular_motion.h -- the motion of what is seen through mirror and glass chains (include/mcpt.h: mcpt_render_motion_ex).
 * Included by csrc/mcpt_temporal.h, beside the projection it ends in; compiled for the device and for the host like the rest of it.
 *
 * Feature sample k of a pixel walks the chain of mcpt_render_aovs_ex (csrc/mcpt_chain.h decides every bounce for both passes).  The
 * terminal hit of the chain is unfolded into a *virtual point*: reflected back across the mirror planes the chain passed, newest first,
 * so that it lies on the primary ray at about the chain's depth; that point is projected through both cameras (tp::sample_motion).
 *
 * State per sample: two affine maps of R^3, A_cur and A_prev, 3 x 4 floats each, row-major (x' = L x + t, t the fourth column), and the
 * number of reflections composed so far; 0 means both maps are "none" and neither is read.
 *   followed reflect bounce   one plane per map, anchor a and unit normal n (the sign of n does not matter):
 *                               triangle  a_cur = tri_point(live record, u, v), a_prev = tri_point(snapshot record, u, v);  n = tri_normal of
 *                                         that record, i.e. from its own e1, e2 by the expression csrc/mcpt_move.h uses at creation, never
 *                                         the stored TriShade::n, so equal records give equal normals bit for bit
 *                               sphere    a_cur = o + d (float)t, a_prev = a_cur + (c_prev - c_cur);  n_cur = n_prev = the chain's normal
 *                             R(a, n)(x) = x - 2 n (n . (x - a)) as a map (reflection);  A <- A o R (compose): the newest reflection
 *                             is applied first, v = R1(R2(... Rk(q)))
 *   followed refract bounce   both maps stay: glass is straight-through
 *   terminal hit              q_cur, q_prev by the first-hit rule of mcpt_render_motion on the last ray and its hit;  v = A(q), or q bit
 *                             for bit while the map is none;  the record is sample_motion(cur, prev, v_cur, v_prev), so
 *                             prev_depth = |v_prev - prev eye|
 *   miss                      {0, 0, 0, 0}
 * All arithmetic is float32 without contraction, dots in the 3-term order x + (y + z).
 *
 * What follows:
 *   - equal cameras and a snapshot equal to the live geometry give dx = dy = 0 bit for bit: both sides evaluate the same expressions on
 *     the same inputs;
 *   - depth 0 has no chain: mcpt_render_motion_ex launches mcpt_render_motion's kernels themselves;
 *   - valid equals the coverage of the chain AOVs whenever both projections have q.z > 0;
 *   - for planar mirrors the virtual point is exact under any rigid motion of object, mirror and camera; for a curved mirror the plane is
 *     the tangent plane at the hit and for glass the bend is ignored: the usual approximations, and the depth test of the blend decides
 *     whether the history they point at is usable.
 */
#ifndef MCPT_SPECULAR_MOTION_H
#define MCPT_SPECULAR_MOTION_H

#ifndef MCPT_TEMPORAL_H
#error "include mcpt_temporal.h, which includes this header after the projection"
#endif

namespace mcpt {
namespace tp {

constexpr int32_t kMaxSpecularMotionDepth = 8;  // dn::kMaxSpecularDepth
constexpr int kMapFloats = 12;                  // one map; a sample carries two

// The unit normal of a triangle record (v0, e1, e2 as tri_point reads it): cross(e1, e2), then z > 0 ? c / sqrtf(z) : c with z = c . c
// (mv::derive_triangle, csrc/mcpt_move.h).
MCPT_TP void tri_normal(const float *g, float n[3]) {
    const float cx = g[4] * g[8] - g[5] * g[7], cy = g[5] * g[6] - g[3] * g[8], cz = g[3] * g[7] - g[4] * g[6];
    const float z = cx * cx + (cy * cy + cz * cz);
    n[0] = z > 0.0f ? cx / sqrtf(z) : cx;
    n[1] = z > 0.0f ? cy / sqrtf(z) : cy;
    n[2] = z > 0.0f ? cz / sqrtf(z) : cz;
}

// R(a, n) as a 3 x 4 map: L = I - (2 n) n^T, t = (2 n) (n . a).
MCPT_TP void reflection(const float a[3], const float n[3], float r[12]) {
    const float d = n[0] * a[0] + (n[1] * a[1] + n[2] * a[2]);
    for (int i = 0; i < 3; ++i) {
        const float n2 = 2.0f * n[i];
        for (int j = 0; j < 3; ++j) r[4 * i + j] = (i == j ? 1.0f : 0.0f) - n2 * n[j];
        r[4 * i + 3] = n2 * d;
    }
}

// A <- A o R: the linear parts multiplied in the 3-term order, t = (L_A t_R) + t_A.  n_refl == 0 (A is none): A = R.
MCPT_TP void compose(float A[12], int32_t n_refl, const float r[12]) {
    if (n_refl == 0) {
        for (int k = 0; k < 12; ++k) A[k] = r[k];
        return;
    }
    float o[12];
    for (int i = 0; i < 3; ++i) {
        const float a0 = A[4 * i], a1 = A[4 * i + 1], a2 = A[4 * i + 2];
        for (int j = 0; j < 3; ++j) o[4 * i + j] = a0 * r[j] + (a1 * r[4 + j] + a2 * r[8 + j]);
        o[4 * i + 3] = (a0 * r[3] + (a1 * r[7] + a2 * r[11])) + A[4 * i + 3];
    }
    for (int k = 0; k < 12; ++k) A[k] = o[k];
}

// v = A(q) = (L q) + t; n_refl == 0: v = q bit for bit.
MCPT_TP void apply_map(const float A[12], int32_t n_refl, const float q[3], float v[3]) {
    if (n_refl == 0) {
        v[0] = q[0], v[1] = q[1], v[2] = q[2];
        return;
    }
    for (int i = 0; i < 3; ++i) v[i] = (A[4 * i] * q[0] + (A[4 * i + 1] * q[1] + A[4 * i + 2] * q[2])) + A[4 * i + 3];
}

// A followed reflect bounce: both maps, each from its own plane.  n_refl counts the reflections composed before this one.
MCPT_TP void chain_reflect(float A_cur[12], float A_prev[12], int32_t n_refl, const float a_cur[3], const float n_cur[3], const float a_prev[3],
                           const float n_prev[3]) {
    float r[12];
    reflection(a_cur, n_cur, r);
    compose(A_cur, n_refl, r);
    reflection(a_prev, n_prev, r);
    compose(A_prev, n_refl, r);
}

// ... on a triangle: the planes of the live record g_cur and of the snapshot's g_prev at the barycentrics (u, v) of the hit.
MCPT_TP void chain_reflect_tri(float A_cur[12], float A_prev[12], int32_t n_refl, const float *g_cur, const float *g_prev, float u, float v) {
    float ac[3], ap[3], nc[3], np[3];
    tri_point(g_cur, u, v, ac);
    tri_point(g_prev, u, v, ap);
    tri_normal(g_cur, nc);
    tri_normal(g_prev, np);
    chain_reflect(A_cur, A_prev, n_refl, ac, nc, ap, np);
}

// ... on a sphere hit at p with the chain's normal n: the tangent plane, moved with the centre.
MCPT_TP void chain_reflect_sphere(float A_cur[12], float A_prev[12], int32_t n_refl, const float p[3], const float n[3], const float c_cur[3],
                                  const float c_prev[3]) {
    const float ap[3] = {p[0] + (c_prev[0] - c_cur[0]), p[1] + (c_prev[1] - c_cur[1]), p[2] + (c_prev[2] - c_cur[2])};
    chain_reflect(A_cur, A_prev, n_refl, p, n, ap, n);
}

// The record of a chain that ends in a hit at q_cur now, q_prev in the snapshot.
MCPT_TP void chain_motion(const Cam &cur, const Cam &prev, const float A_cur[12], const float A_prev[12], int32_t n_refl, const float q_cur[3],
                          const float q_prev[3], float out[4]) {
    float vc[3], vp[3];
    apply_map(A_cur, n_refl, q_cur, vc);
    apply_map(A_prev, n_refl, q_prev, vp);
    sample_motion(cur, prev, vc, vp, out);
}

}  // namespace tp
}  // namespace mcpt

#endif  // MCPT_SPECULAR_MOTION_H
