/*
 * mcpt_move.h -- the arithmetic of moving an object and of deriving a triangle's records from its vertices (include/mcpt.h:
 * mcpt_scene_update, mcpt_transform_triangles, mcpt_scene_deform, mcpt_deform_triangles).
 *
 * Every function here is callable from the host and from the device.  The scene builder (csrc/mcpt_scene.cpp), the host helper
 * mcpt_transform_triangles and the update kernel (csrc/mcpt_update.hip) all compile these expressions, so a triangle moved on the device
 * gets the records a fresh scene would give it bit for bit: float32 arithmetic in a fixed order, no FMA contraction
 * (-ffp-contract=off), correctly rounded f32 division and square root on both sides.
 */
#ifndef MCPT_MOVE_H
#define MCPT_MOVE_H

#include "mcpt_internal.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MCPT_MV static __host__ __device__ __forceinline__
#else
#include <math.h>
#define MCPT_MV static inline
#endif

namespace mcpt {
namespace mv {

struct V3 {
    float x, y, z;
};
MCPT_MV V3 ld(const float *p) { return {p[0], p[1], p[2]}; }
MCPT_MV V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
MCPT_MV float dot3(V3 a, V3 b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }  // Eigen's 3-term redux order
MCPT_MV V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// p' = M p + t for a row-major 3x4 matrix: the 3-term dot order, then the translation.
MCPT_MV V3 move_point(const float *m, V3 p) {
    return {(m[0] * p.x + (m[1] * p.y + m[2] * p.z)) + m[3], (m[4] * p.x + (m[5] * p.y + m[6] * p.z)) + m[7],
            (m[8] * p.x + (m[9] * p.y + m[10] * p.z)) + m[11]};
}

// What Triangle::Triangle derives from the stored vertices (Triangle.hpp:50-56): the edges, the normal and the area.
struct TriDerived {
    V3 e1, e2, n;
    float area;
};
MCPT_MV TriDerived derive_triangle(V3 v0, V3 v1, V3 v2) {
    TriDerived d;
    d.e1 = sub(v1, v0);
    d.e2 = sub(v2, v0);  // Triangle.hpp:52-55
    const V3 c = cross3(d.e1, d.e2);
    const float z = dot3(c, c);
    d.n = z > 0.f ? V3{c.x / sqrtf(z), c.y / sqrtf(z), c.z / sqrtf(z)} : c;
    d.area = sqrtf(dot3(c, c)) * 0.5f;
    return d;
}

// The geometry words of the two per-triangle records; mat_bits, mat, the texture coordinates and the padding are the caller's.
MCPT_MV void store_geom(TriGeom &g, V3 v0, const TriDerived &d) {
    g.v0[0] = v0.x;
    g.v0[1] = v0.y;
    g.v0[2] = v0.z;
    g.e1x = d.e1.x;
    g.e1yz[0] = d.e1.y;
    g.e1yz[1] = d.e1.z;
    g.e2xy[0] = d.e2.x;
    g.e2xy[1] = d.e2.y;
    g.e2z = d.e2.z;
}

MCPT_MV void move_triangle(const float *m, const mcpt_triangle &in, mcpt_triangle &out) {
    const V3 a = move_point(m, ld(in.v0)), b = move_point(m, ld(in.v1)), c = move_point(m, ld(in.v2));
    const float uv[6] = {in.t0[0], in.t0[1], in.t1[0], in.t1[1], in.t2[0], in.t2[1]};  // (in and out may be one triangle)
    out.v0[0] = a.x;
    out.v0[1] = a.y;
    out.v0[2] = a.z;
    out.v1[0] = b.x;
    out.v1[1] = b.y;
    out.v1[2] = b.z;
    out.v2[0] = c.x;
    out.v2[1] = c.y;
    out.v2[2] = c.z;
    out.t0[0] = uv[0];
    out.t0[1] = uv[1];
    out.t1[0] = uv[2];
    out.t1[1] = uv[3];
    out.t2[0] = uv[4];
    out.t2[1] = uv[5];
}

// Deformation (mcpt_scene_deform): the new base triangle is `in` with its nine position floats replaced by p[0..9) = v0, v1, v2, bit for
// bit (a copy, no arithmetic: the sign of a zero survives); the texture coordinates are in's.
MCPT_MV void deform_triangle(const float *p, const mcpt_triangle &in, mcpt_triangle &out) {
    const float uv[6] = {in.t0[0], in.t0[1], in.t1[0], in.t1[1], in.t2[0], in.t2[1]};  // (in and out may be one triangle)
    for (int k = 0; k < 3; ++k) {
        out.v0[k] = p[k];
        out.v1[k] = p[3 + k];
        out.v2[k] = p[6 + k];
    }
    out.t0[0] = uv[0];
    out.t0[1] = uv[1];
    out.t1[0] = uv[2];
    out.t1[1] = uv[3];
    out.t2[0] = uv[4];
    out.t2[1] = uv[5];
}

// True when all nine position floats are finite (a NaN fails every comparison).
MCPT_MV bool positions_finite(const float *p) {
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && (p[k] - p[k] == 0.f);
    return ok;
}

}  // namespace mv
}  // namespace mcpt

#endif /* MCPT_MOVE_H */
