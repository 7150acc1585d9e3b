// Moving and deforming objects in a live scene (include/mcpt.h: mcpt_scene_update, mcpt_scene_deform): the kernels of the device path,
// the kernel that rewrites the material words of primitives (mcpt_scene_set_materials), the kernel that writes the whole records of
// added primitives (mcpt_scene_add_objects),
// and the host helpers mcpt_transform_triangles and mcpt_deform_triangles.  The scene-level part (argument checks, the two paths, the swap of the new arrays) is beside
// mcpt_scene_create in csrc/mcpt_upload.hip; the arithmetic is csrc/mcpt_move.h, shared with the scene builder.
#include <cmath>

#include "mcpt_host.h"
#include "mcpt_move.h"

namespace mcpt {

namespace {

constexpr int kB = 256;

// The moved triangle `t` of primitive `ti`, for the tree builder and into the geometry words of the two 48-byte records: 16-byte loads and
// stores of whole quarters, so that mat_bits, mat, the texture coordinates and the padding pass through untouched.
__device__ __forceinline__ void write_triangle(const mcpt_triangle &t, int32_t ti, mcpt_triangle *__restrict__ tris_cur, TriGeom *__restrict__ tri_geom,
                                               TriShade *__restrict__ tri_shade) {
    tris_cur[ti] = t;
    const mv::V3 v0 = mv::ld(t.v0);
    const mv::TriDerived D = mv::derive_triangle(v0, mv::ld(t.v1), mv::ld(t.v2));
    float4 *g = reinterpret_cast<float4 *>(tri_geom + ti);
    float4 g2 = g[2];  // {e2z, mat_bits, pad, pad}
    g2.x = D.e2.z;
    g[0] = make_float4(v0.x, v0.y, v0.z, D.e1.x);
    g[1] = make_float4(D.e1.y, D.e1.z, D.e2.x, D.e2.y);
    g[2] = g2;
    float4 *s = reinterpret_cast<float4 *>(tri_shade + ti);
    float4 s0 = s[0];  // {n.xyz, mat}
    s0.x = D.n.x;
    s0.y = D.n.y;
    s0.z = D.n.z;
    s[0] = s0;
}

// One lane per triangle of the moved meshes (and one per moved sphere).  The lane finds its segment by bisection over first_lane, reads
// the BASE triangle (transforms are absolute), and writes the moved triangle (write_triangle).
__global__ __launch_bounds__(kB) void k_move_objects(const MoveSeg *__restrict__ segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *__restrict__ tris0,
                                                      mcpt_triangle *__restrict__ tris_cur, TriGeom *__restrict__ tri_geom, TriShade *__restrict__ tri_shade,
                                                      SphereRec *__restrict__ spheres) {
    const int32_t lane = (int32_t)(blockIdx.x * kB + threadIdx.x);
    if (lane >= n_lanes) return;
    int32_t lo = 0, hi = n_segs - 1;  // the last segment whose first_lane <= lane
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].first_lane <= lane) lo = mid;
        else hi = mid - 1;
    }
    const MoveSeg *sg = segs + lo;
    const float4 r0 = *reinterpret_cast<const float4 *>(sg->m), r1 = *reinterpret_cast<const float4 *>(sg->m + 4), r2 = *reinterpret_cast<const float4 *>(sg->m + 8);
    const float m[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    const bool raw = sg->raw != 0;
    if (sg->first_tri < 0) {  // a sphere: the centre moves, the radius stays
        const mv::V3 c0 = {sg->c0[0], sg->c0[1], sg->c0[2]};
        const mv::V3 c = raw ? c0 : mv::move_point(m, c0);
        float4 *rec = reinterpret_cast<float4 *>(spheres + sg->object);
        float4 q = rec[0];  // {c.xyz, radius}
        q.x = c.x;
        q.y = c.y;
        q.z = c.z;
        rec[0] = q;
        return;
    }
    const int32_t ti = sg->first_tri + (lane - sg->first_lane);
    mcpt_triangle t = tris0[ti];
    if (!raw) mv::move_triangle(m, t, t);
    write_triangle(t, ti, tris_cur, tri_geom, tri_shade);
}

// One lane per triangle of the deformed meshes (mcpt_scene_deform).  The lane reads its nine position floats (36-byte stride: a wave's 64
// triangles are one contiguous 2304-byte run of the staging buffer or of the caller's device array), raises the flag word when one is
// not finite, forms the new base triangle (texture coordinates from the base it replaces) into the aside array `base`, applies the
// object's transform unless `raw`, and writes the builder's triangle and the records as k_move_objects does.
__global__ __launch_bounds__(kB) void k_deform_objects(const DeformSeg *__restrict__ segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *__restrict__ tris0,
                                                        mcpt_triangle *__restrict__ base, mcpt_triangle *__restrict__ tris_cur, TriGeom *__restrict__ tri_geom,
                                                        TriShade *__restrict__ tri_shade, uint32_t *__restrict__ flag) {
    const int32_t lane = (int32_t)(blockIdx.x * kB + threadIdx.x);
    if (lane >= n_lanes) return;
    int32_t lo = 0, hi = n_segs - 1;  // the last segment whose first_lane <= lane
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].first_lane <= lane) lo = mid;
        else hi = mid - 1;
    }
    const DeformSeg *sg = segs + lo;
    const int32_t k = lane - sg->first_lane;
    const float *p = sg->positions + (size_t)k * 9;
    const float q[9] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]};
    if (!mv::positions_finite(q)) {  // the call is refused: the aside arrays are dropped, nothing else needs writing
        *flag = 1u;
        return;
    }
    const int32_t ti = sg->first_tri + k;
    mcpt_triangle t;
    mv::deform_triangle(q, tris0[ti], t);
    base[ti] = t;
    if (sg->raw == 0) {
        const float4 r0 = *reinterpret_cast<const float4 *>(sg->m), r1 = *reinterpret_cast<const float4 *>(sg->m + 4), r2 = *reinterpret_cast<const float4 *>(sg->m + 8);
        const float m[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        mv::move_triangle(m, t, t);
    }
    write_triangle(t, ti, tris_cur, tri_geom, tri_shade);
}

// One lane per primitive whose material words change (mcpt_scene_set_materials, path 2): the triangles of the affected meshes and one lane
// per affected sphere.  The lane finds its segment by the bisection of k_move_objects and stores the segment's two words: single dword
// stores, so that everything else in the records stays bit for bit without being read (a 16-byte quarter would need a load, a wait and
// four times the bytes for the same number of store instructions).
__global__ __launch_bounds__(kB) void k_set_materials(const mat::MatSeg *__restrict__ segs, int32_t n_segs, int32_t n_lanes, TriGeom *__restrict__ tri_geom,
                                                       TriShade *__restrict__ tri_shade, SphereRec *__restrict__ spheres) {
    const int32_t lane = (int32_t)(blockIdx.x * kB + threadIdx.x);
    if (lane >= n_lanes) return;
    int32_t lo = 0, hi = n_segs - 1;  // the last segment whose first_lane <= lane
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].first_lane <= lane) lo = mid;
        else hi = mid - 1;
    }
    const uint4 a = *reinterpret_cast<const uint4 *>(segs + lo);        // {first_lane, count, first_tri, object}
    const uint2 b = *(reinterpret_cast<const uint2 *>(segs + lo) + 2);  // {mat_bits, mat}
    const int32_t k = lane - (int32_t)a.x;
    if (k >= (int32_t)a.y) return;  // (never for a table whose segments tile the lanes)
    if ((int32_t)a.z < 0) {
        SphereRec *rec = spheres + (int32_t)a.w;
        rec->mat = (int32_t)b.y;
        rec->mat_bits = b.x;
        return;
    }
    const int32_t ti = (int32_t)a.z + k;
    tri_geom[ti].mat_bits = b.x;
    tri_shade[ti].mat = (int32_t)b.y;
}

// One lane per added triangle and one per added sphere (mcpt_scene_add_objects, path 1).  The lane finds its segment by the bisection of
// k_move_objects.  A triangle lane reads its triangle from the appended tail of the base array, stores it for the tree builder and
// writes the WHOLE TriGeom and TriShade records -- the geometry words by mv::derive_triangle in the order of mv::store_geom, mat_bits, the
// normal, mat, the six texture coordinates, and zeros for the padding as the host's memset leaves it -- with three 16-byte stores each
// and no load: the records are 48 bytes on 16-byte boundaries, and a quarter is the widest store the hardware has.  A sphere lane
// writes its whole SphereRec with two.  Integer words go through uint4, so no bit of them passes through a float register type.
__global__ __launch_bounds__(kB) void k_add_objects(const AddSeg *__restrict__ segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *__restrict__ tris0,
                                                     mcpt_triangle *__restrict__ tris_cur, TriGeom *__restrict__ tri_geom, TriShade *__restrict__ tri_shade,
                                                     SphereRec *__restrict__ spheres) {
    const int32_t lane = (int32_t)(blockIdx.x * kB + threadIdx.x);
    if (lane >= n_lanes) return;
    int32_t lo = 0, hi = n_segs - 1;  // the last segment whose first_lane <= lane
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].first_lane <= lane) lo = mid;
        else hi = mid - 1;
    }
    const uint4 a = *reinterpret_cast<const uint4 *>(segs + lo);        // {first_lane, count, first_tri, object}
    const uint4 b = *(reinterpret_cast<const uint4 *>(segs + lo) + 1);  // {mat_bits, mat, radius, pad}
    const int32_t k = lane - (int32_t)a.x;
    if (k >= (int32_t)a.y) return;  // (never for a table whose segments tile the lanes)
    if ((int32_t)a.z < 0) {
        const uint4 c = *(reinterpret_cast<const uint4 *>(segs + lo) + 2);  // {c.xyz, pad}
        const float radius = __uint_as_float(b.z);
        uint4 *rec = reinterpret_cast<uint4 *>(spheres + (int32_t)a.w);
        rec[0] = make_uint4(c.x, c.y, c.z, b.z);                                   // {c.xyz, radius}
        rec[1] = make_uint4(__float_as_uint(radius * radius), b.y, b.x, 0u);       // {radius2, mat, mat_bits, pad}
        return;
    }
    const int32_t ti = (int32_t)a.z + k;
    const mcpt_triangle t = tris0[ti];
    tris_cur[ti] = t;
    const mv::V3 v0 = mv::ld(t.v0);
    const mv::TriDerived D = mv::derive_triangle(v0, mv::ld(t.v1), mv::ld(t.v2));
    const auto u = [](float f) { return __float_as_uint(f); };
    uint4 *g = reinterpret_cast<uint4 *>(tri_geom + ti);
    g[0] = make_uint4(u(v0.x), u(v0.y), u(v0.z), u(D.e1.x));
    g[1] = make_uint4(u(D.e1.y), u(D.e1.z), u(D.e2.x), u(D.e2.y));
    g[2] = make_uint4(u(D.e2.z), b.x, 0u, 0u);  // {e2z, mat_bits, pad, pad}
    uint4 *s = reinterpret_cast<uint4 *>(tri_shade + ti);
    s[0] = make_uint4(u(D.n.x), u(D.n.y), u(D.n.z), b.y);  // {n.xyz, mat}
    s[1] = make_uint4(u(t.t0[0]), u(t.t0[1]), u(t.t1[0]), u(t.t1[1]));
    s[2] = make_uint4(u(t.t2[0]), u(t.t2[1]), 0u, 0u);  // {t2, pad, pad}
}

}  // namespace

void launch_add_objects(const AddSeg *d_segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *tris0, mcpt_triangle *tris_cur, TriGeom *tri_geom,
                        TriShade *tri_shade, SphereRec *spheres, hipStream_t s) {
    if (n_lanes <= 0 || n_segs <= 0) return;
    hipLaunchKernelGGL(k_add_objects, dim3((uint32_t)((n_lanes + kB - 1) / kB)), dim3(kB), 0, s, d_segs, n_segs, n_lanes, tris0, tris_cur, tri_geom, tri_shade,
                       spheres);
}

void launch_move_objects(const MoveSeg *d_segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *tris0, mcpt_triangle *tris_cur, TriGeom *tri_geom,
                         TriShade *tri_shade, SphereRec *spheres, hipStream_t s) {
    if (n_lanes <= 0 || n_segs <= 0) return;
    hipLaunchKernelGGL(k_move_objects, dim3((uint32_t)((n_lanes + kB - 1) / kB)), dim3(kB), 0, s, d_segs, n_segs, n_lanes, tris0, tris_cur, tri_geom, tri_shade,
                       spheres);
}

void launch_deform_objects(const DeformSeg *d_segs, int32_t n_segs, int32_t n_lanes, const mcpt_triangle *tris0, mcpt_triangle *base, mcpt_triangle *tris_cur,
                           TriGeom *tri_geom, TriShade *tri_shade, uint32_t *flag, hipStream_t s) {
    if (n_lanes <= 0 || n_segs <= 0) return;
    hipLaunchKernelGGL(k_deform_objects, dim3((uint32_t)((n_lanes + kB - 1) / kB)), dim3(kB), 0, s, d_segs, n_segs, n_lanes, tris0, base, tris_cur, tri_geom,
                       tri_shade, flag);
}

void launch_set_materials(const mat::MatSeg *d_segs, int32_t n_segs, int32_t n_lanes, TriGeom *tri_geom, TriShade *tri_shade, SphereRec *spheres, hipStream_t s) {
    if (n_lanes <= 0 || n_segs <= 0) return;
    hipLaunchKernelGGL(k_set_materials, dim3((uint32_t)((n_lanes + kB - 1) / kB)), dim3(kB), 0, s, d_segs, n_segs, n_lanes, tri_geom, tri_shade, spheres);
}

}  // namespace mcpt

extern "C" int mcpt_deform_triangles(int64_t n, const float *positions, const mcpt_triangle *in, mcpt_triangle *out) {
    using namespace mcpt;
    if (n < 0 || (n > 0 && (!positions || !in || !out))) return fail(MCPT_ERR_ARG, "mcpt_deform_triangles: bad argument");
    for (int64_t i = 0; i < n; ++i) mv::deform_triangle(positions + i * 9, in[i], out[i]);
    return MCPT_OK;
}

extern "C" int mcpt_transform_triangles(const float m[12], int64_t n, const mcpt_triangle *in, mcpt_triangle *out) {
    using namespace mcpt;
    if (!m || n < 0 || (n > 0 && (!in || !out))) return fail(MCPT_ERR_ARG, "mcpt_transform_triangles: bad argument");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(m[k])) return fail(MCPT_ERR_ARG, "mcpt_transform_triangles: a matrix entry is not finite");
    for (int64_t i = 0; i < n; ++i) mv::move_triangle(m, in[i], out[i]);
    return MCPT_OK;
}
