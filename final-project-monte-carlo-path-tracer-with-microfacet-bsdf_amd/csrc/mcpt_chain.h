// The bounce decision of a specular chain (include/mcpt.h: mcpt_render_aovs_ex, mcpt_render_motion_ex), once, for the two kernels that walk
// the chains: k_aov_chain (csrc/mcpt_denoise.hip) and k_motion_chain (csrc/mcpt_temporal.hip).  Both call these functions with the same
// ray, hit and normal, so the two passes cannot disagree on a path.
#pragma once
#include "mcpt_device.h"

namespace mcpt {

MCPT_DI uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// The hit distance of a closest-hit record {t lo, t hi, prim, mat_bits}
MCPT_DI double hit_t(const uint4 &h) { return __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x)); }

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
