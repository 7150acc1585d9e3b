// The bounce decision of a specular chain (include/mcpt.h: mcpt_render_aovs_ex, mcpt_render_motion_ex, mcpt_render_probe_lit), once, for the
// kernels that walk the chains: k_aov_chain (csrc/mcpt_denoise.hip), k_motion_chain (csrc/mcpt_temporal.hip) and k_lit_terminal
// (csrc/mcpt_probes.hip).  All call these functions with the same ray, hit and normal, so the passes cannot disagree on a path.
#pragma once
#include "mcpt_device.h"

namespace mcpt {

MCPT_DI uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// The hit distance of a closest-hit record {t lo, t hi, prim, mat_bits}
MCPT_DI double hit_t(const uint4 &h) { return __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x)); }

// Normal, uv and albedo of a hit as the shading reads them (k_shade), once, for the kernels that record a sample's features: k_aov_resolve
// and k_aov_chain (csrc/mcpt_denoise.hip) and k_lit_terminal (csrc/mcpt_probes.hip).  ro / rd is the ray, p = ro + rd * (float)t its hit
// point.  nrm is the normal as stored (not flipped); uv comes from the recorded hit's barycentrics for textured triangles and is 0 otherwise.
MCPT_DI void hit_surface(const DevScene &S, int32_t prim, uint32_t mat_bits, f3 ro, f3 rd, f3 p, f3 &nrm, f2 &uv) {
    uv = f2{0.f, 0.f};
    if (prim < S.n_tri) {
        const TriShade ts = S.tri_shade[prim];
        nrm = mk3(ts.n[0], ts.n[1], ts.n[2]);
        if (mat_bits & kMatTextured) {
            double tt, u, v;
            const Ray rr = make_ray(ro, rd);
            if (tri_hit(S.tri_geom[prim], rr, tt, u, v)) {
                const float a = (float)(1 - u - v), b = (float)u, c = (float)v;
                uv.x = a * ts.t0[0] + b * ts.t1[0] + c * ts.t2[0];
                uv.y = a * ts.t0[1] + b * ts.t1[1] + c * ts.t2[1];
            }
        }
    } else {
        const SphereRec sp = S.spheres[prim - S.n_tri];
        nrm = normalized(p - mk3(sp.c[0], sp.c[1], sp.c[2]));
    }
}

// Material.hpp:134-151 for conductors; 1 for dielectrics and emitters.
MCPT_DI void hit_albedo(const MaterialRec &M, uint32_t mat_bits, f2 uv, float alb[3]) {
    alb[0] = alb[1] = alb[2] = 1.f;
    if (!(mat_bits >> 31) && (M.type == MCPT_SMOOTH_CONDUCTOR || M.type == MCPT_ROUGH_CONDUCTOR)) {
        alb[0] = get_reflectance(M, uv, 0);
        alb[1] = get_reflectance(M, uv, 1);
        alb[2] = get_reflectance(M, uv, 2);
    }
}

// The stop rule: a sample that has followed b bounces goes on from a vertex of material M iff b < max_b, M is Dirac and not an emitter.
MCPT_DI bool chain_continues(const MaterialRec &M, uint32_t mat_bits, int32_t b, int32_t max_b) { return b < max_b && M.isDirac && !(mat_bits >> 31); }

// The bounce at a vertex that continues: k_shade's vertex (Scene.cpp:109-159) with mfn = n, channel 1, the more likely branch.  rd is the
// ray's direction, p the hit point, nrm the geometric normal as stored (not flipped).  Returns whether the sample reflects; p2 and wi are the
// origin and the direction of its next ray.
MCPT_DI bool chain_bounce(const MaterialRec &M, f3 rd, f3 p, f3 nrm, f3 &p2, f3 &wi) {
    const f3 wo = -rd;
    const float kr = mat_fresnel(M, rd, nrm, 1);
    const bool isReflect = kr > 0.5f;
    if (isReflect) p2 = (dot(wo, nrm) < 0) ? (p - nrm * kEps) : (p + nrm * kEps);
    else p2 = (dot(wo, nrm) < 0) ? (p + nrm * kEps) : (p - nrm * kEps);
    wi = isReflect ? mat_reflect(wo, nrm) : mat_refract(M, rd, nrm, 1);
    return isReflect;
}

}  // namespace mcpt
