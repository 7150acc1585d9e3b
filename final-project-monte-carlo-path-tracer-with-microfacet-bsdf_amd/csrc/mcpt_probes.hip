// Light probes (include/mcpt.h: mcpt_query_probes, mcpt_probe_rays, mcpt_probe_shade, mcpt_bake_probe_grid and the host-only
// mcpt_sh_basis_host / mcpt_sh_irradiance_host / mcpt_probe_grid_points_host / mcpt_probe_shade_host).  csrc/mcpt_sh.h states the rule --
// basis, irradiance, grid lookup -- once; the whole-sphere first ray is sensor_ray's third branch (csrc/mcpt_sensor.h) and the projection
// fold k_accumulate_sh sits beside k_accumulate (csrc/mcpt_kernels.hip), launched by render_list at both of its accumulate sites.
//
// Kernels here, on the caller's stream:
//   k_probe_grid_points  one lane per probe: sh::grid_point into the scene-owned point buffer (mcpt_bake_probe_grid)
//   k_probe_shade        one lane per (point, normal): sh::probe_shade from the coefficient buffer; eight 108-byte rows are read per lane
//
// Probe visibility (mcpt_query_probe_depth, mcpt_probe_shade_visible, mcpt_bake_probe_volume and their host forms; csrc/mcpt_probe_depth.h
// states the rule).  Per chunk of the ray queries' staging buffers (QueryBufs, csrc/mcpt_host.h; piece_cut of csrc/mcpt_direct.h cuts this
// query and the direct term below into chunks, and sizes the staging), on the caller's stream:
//   k_probe_depth_rays     one lane per (probe, sample): sensor_ray's whole-sphere ray straight into the staged float4 arrays, tmax = +inf
//   closest hits           launch_trace_closest on the staged chunk, as run_query (csrc/mcpt_rayquery.hip) runs it: no second tree walk
//   k_probe_depth_fold     one wave per probe, lane = texel of the 8 x 8 map: per block of 64 samples lane l prepares sample l (hit word,
//                          distance, the normal k_query_resolve reports, back-face flag; the block's back-face count is a ballot), then
//                          the wave walks the block in sample order with (d, r) broadcast from lane s by a wave-uniform lane read, and
//                          every lane adds to its texel's three sums in registers
//   k_probe_shade_visible  one lane per (point, normal): pd::shade_visible
// Every store is a plain vector store; nothing above uses atomics, LDS, scratch or inline assembly.
//
// Relighting a probe volume (mcpt_probe_volume_relight; csrc/mcpt_probe_relight.h states the fold and the blend).  Per piece of the ray
// queries' staging buffers, as the depth query cuts them:
//   k_probe_depth_rays, closest hits   as above: the probes' whole-sphere rays and their hits, staged once
//   k_lit_terminal (b = 0, max_b = 0)  the lit sample's records {v or a, kind} {nf} {p} into scene-owned buffers (ProbeBufs, csrc/mcpt_host.h)
//   direct_term                        when asked: D per record, through shadow-ray staging of its own, keys (probe, sample_offset + k)
//   k_lit_shade                        the lookup in the previous volume: r0.xyz = a * (max(E, 0) + D)
//   k_probe_relight_fold               one wave per probe, lane = (coefficient, channel): the 27 sums in sample order and, at a probe's last
//                                      piece, the blend with the previous coefficients
//   k_probe_depth_fold                 when depth outputs are given: from the same staged hits
// The new kernel uses plain vector stores, no atomics, no LDS and no scratch.
//
// Probe-lit frames (mcpt_render_probe_lit; lit_pass in csrc/mcpt_render.hip runs them per chunk of the AOV pass's chunk loop):
//   k_lit_terminal  one lane per ray of a list: the chain step of k_aov_chain; a sample that stops records {v or a, kind} {nf} {p}
//   k_lit_shade     one lane per sample: the grid lookup (plain or occlusion-aware) of a sample that ended on a surface
//   k_lit_fold      one lane per pixel, in sample order
// Their only atomics are integer ones, one per wave: the next list's length (as k_aov_chain) and the count of lookups.
//
// The sampled direct term (mcpt_query_direct; csrc/mcpt_direct.h states the rule).  Per chunk of the ray queries' staging buffers:
//   k_direct_rays   (csrc/mcpt_kernels.hip, beside sample_light) one lane per (point, light sample): Philox block, sample_light,
//                   dl::sample_geometry; the record of the sample, and the shadow ray of a live one appended to the compacted ray list
//   closest hits    launch_trace_closest over that list, its length read on the device: a dead sample costs no traversal
//   k_direct_fold   one lane per point, in sample order: the visibility window in double, the sum, and at a point's last sample / pi
#include <cmath>

#include "mcpt_chain.h"
#include "mcpt_direct.h"
#include "mcpt_frame.h"
#include "mcpt_host.h"
#include "mcpt_probe_depth.h"
#include "mcpt_probe_relight.h"
#include "mcpt_sh.h"

using namespace mcpt;

namespace mcpt {
namespace {

constexpr int kPbBlock = 256;  // 4 waves

__global__ __launch_bounds__(kPbBlock) void k_probe_grid_points(sh::Grid g, uint32_t n, float *__restrict__ points) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t nx = (uint32_t)g.dims[0], ny = (uint32_t)g.dims[1];
    const uint32_t ix = i % nx, r = i / nx;
    float p[3];
    sh::grid_point(g, (int32_t)ix, (int32_t)(r % ny), (int32_t)(r / ny), p);
    points[3 * (size_t)i] = p[0];
    points[3 * (size_t)i + 1] = p[1];
    points[3 * (size_t)i + 2] = p[2];
}

__global__ __launch_bounds__(kPbBlock) void k_probe_shade(sh::Grid g, const float *__restrict__ coef, uint32_t n, const float *__restrict__ points,
                                                        const float *__restrict__ normals, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n) return;
    const size_t q = 3 * (size_t)i;
    const float p[3] = {points[q], points[q + 1], points[q + 2]}, nr[3] = {normals[q], normals[q + 1], normals[q + 2]};
    float e[3];
    sh::probe_shade(g, coef, p, nr, e);
    out[q] = e[0];
    out[q + 1] = e[1];
    out[q + 2] = e[2];
}

// The whole-sphere first rays of probes i0 .. i0 + m - 1, samples k_first .. k_first + kc - 1 (absolute), probe-major into the staging.
__global__ __launch_bounds__(kPbBlock) void k_probe_depth_rays(const float *__restrict__ origins, uint32_t seed, uint32_t i0, uint32_t kc, uint32_t k_first,
                                                             uint32_t n, float4 *__restrict__ ray_o, float4 *__restrict__ ray_d) {
    const uint32_t g = blockIdx.x * kPbBlock + threadIdx.x;
    if (g >= n) return;
    const uint32_t pi = g / kc, s = g - pi * kc;
    f3 pos, dir;
    sensor_ray(SensorConst{origins, nullptr, kSensorSphere}, seed, i0 + pi, k_first + s, pos, dir);
    ray_o[g] = make_float4(pos.x, pos.y, pos.z, 0.f);
    ray_d[g] = make_float4(dir.x, dir.y, dir.z, INFINITY);
}

MCPT_DI float lane_read(float v, uint32_t lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane)); }

// load: the sums and counts of these probes continue what the buffers hold (accumulate, or a later chunk of one probe's samples).
__global__ __launch_bounds__(kPbBlock) void k_probe_depth_fold(DevScene S, const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d,
                                                             const uint4 *__restrict__ hit, uint32_t i0, uint32_t m, uint32_t kc, int load,
                                                             float max_distance, float *__restrict__ moments, int32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pi = blockIdx.x * (kPbBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pi >= m) return;  // (wave-uniform)
    const size_t i = (size_t)i0 + pi;
    float c[3];
    pd::texel_dir((int32_t)lane, c);
    float *dst = moments + (i * (size_t)pd::kTexels + lane) * 3;
    float W = 0.f, S1 = 0.f, S2 = 0.f;
    if (load) {
        W = dst[0];
        S1 = dst[1];
        S2 = dst[2];
    }
    const size_t base = (size_t)pi * kc;
    uint32_t back = 0;
    for (uint32_t kb = 0; kb < kc; kb += 64u) {
        const uint32_t cnt = kc - kb < 64u ? kc - kb : 64u;
        float dx = 0.f, dy = 0.f, dz = 0.f, r = max_distance;
        bool bf = false;
        if (lane < cnt) {
            const size_t g = base + kb + lane;
            const uint4 h = hit[g];
            const float4 d4 = ray_d[g];
            dx = d4.x, dy = d4.y, dz = d4.z;
            const int32_t prim = (int32_t)h.z;
            if (prim >= 0) {
                const double t = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
                f3 nrm;
                if (prim < S.n_tri) {
                    const float4 q = *reinterpret_cast<const float4 *>(S.tri_shade + prim);  // {n.xyz, mat}
                    nrm = mk3(q.x, q.y, q.z);
                } else {
                    const float4 sp = *reinterpret_cast<const float4 *>(S.spheres + (prim - S.n_tri));  // {c.xyz, radius}
                    const float4 o4 = ray_o[g];
                    const f3 p = mk3(o4.x, o4.y, o4.z) + mk3(dx, dy, dz) * (float)t;
                    nrm = normalized(p - mk3(sp.x, sp.y, sp.z));
                }
                r = fminf((float)t, max_distance);
                bf = dot(nrm, mk3(dx, dy, dz)) > 0.f;
            }
        }
        back += (uint32_t)__popcll(__ballot(bf));
        for (uint32_t s = 0; s < cnt; ++s) {  // (a uniform bound: the tail of a short block is not walked)
            const float d[3] = {lane_read(dx, s), lane_read(dy, s), lane_read(dz, s)};
            pd::fold_sample(pd::fold_weight(c, d), lane_read(r, s), W, S1, S2);
        }
    }
    dst[0] = W;
    dst[1] = S1;
    dst[2] = S2;
    if (lane == 0) {
        int32_t *cn = counts + 2 * i;
        const int32_t n0 = load ? cn[0] : 0, b0 = load ? cn[1] : 0;
        cn[0] = n0 + (int32_t)kc;
        cn[1] = b0 + (int32_t)back;
    }
}

__global__ __launch_bounds__(kPbBlock) void k_probe_shade_visible(sh::Grid g, const float *__restrict__ coef, const float *__restrict__ moments,
                                                                const int32_t *__restrict__ counts, float normal_bias, float backface_max, uint32_t n,
                                                                const float *__restrict__ points, const float *__restrict__ normals,
                                                                float *__restrict__ out, float *__restrict__ weight_out) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n) return;
    const size_t q = 3 * (size_t)i;
    const float p[3] = {points[q], points[q + 1], points[q + 2]}, nr[3] = {normals[q], normals[q + 1], normals[q + 2]};
    float e[3], A;
    pd::shade_visible(g, coef, moments, counts, normal_bias, backface_max, p, nr, e, &A);
    out[q] = e[0];
    out[q + 1] = e[1];
    out[q + 2] = e[2];
    if (weight_out) weight_out[i] = A;
}

// Samples s < jc of the points i0 .. i0 + m - 1 folded into out (`stride` floats per point).  load: the sums continue what out holds (an earlier piece of the same
// points' samples); last: these are the points' last samples, so the sums are divided by pi.
__global__ __launch_bounds__(kPbBlock) void k_direct_fold(uint32_t i0, uint32_t m, uint32_t jc, int load, int last, const float4 *__restrict__ slot,
                                                        const float4 *__restrict__ ray_d, const uint4 *__restrict__ hit, float *__restrict__ out,
                                                        uint32_t stride) {
    const uint32_t pi = blockIdx.x * kPbBlock + threadIdx.x;
    if (pi >= m) return;
    float *o = out + (size_t)stride * ((size_t)i0 + pi);
    float acc[3] = {0.f, 0.f, 0.f};
    if (load) acc[0] = o[0], acc[1] = o[1], acc[2] = o[2];
    const float4 *row = slot + (size_t)pi * jc;
    for (uint32_t s = 0; s < jc; ++s) {
        const float4 r = row[s];
        const uint32_t k = __float_as_uint(r.w);
        if (k == kDirectDead) continue;
        const uint4 h = hit[k];
        if ((int32_t)h.z < 0 || !dl::in_window(hit_t(h), ray_d[k].w)) continue;
        const float c[3] = {r.x, r.y, r.z};
        dl::fold_sample(c, acc);
    }
    if (last) dl::fold_end(acc, acc);
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
}

// How a lit sample ended (r0[j].w of the lit pass's records, as bits).
constexpr uint32_t kLitMiss = 0u, kLitEmitter = 1u, kLitSurface = kLitSurfaceKind;

// One step of the lit pass's chains: k_aov_chain (csrc/mcpt_denoise.hip) with the lit sample's records in place of the AOV record.  A
// sample that stops writes r0[j] = {v or a, kind}, r1[j] = {nf, 0}, r2[j] = {p, 0}: for a miss and an emitter v is the sample's final
// value, for any other hit a = thr * albedo waits for k_lit_shade.  A sample that follows a Dirac bounce (b < max_b) appends its next ray
// and state to the next list (ballot + prefix count, one atomic per wave on n_next).
__global__ __launch_bounds__(kPbBlock) void k_lit_terminal(DevScene S, uint32_t n, int32_t b, int32_t max_b, const float4 *__restrict__ ray_o,
                                                         const float4 *__restrict__ ray_d, const uint4 *__restrict__ hit,
                                                         const float4 *__restrict__ chain_in, float4 *__restrict__ r0, float4 *__restrict__ r1,
                                                         float4 *__restrict__ r2, float4 *__restrict__ next_o, float4 *__restrict__ next_d,
                                                         float4 *__restrict__ chain_out, uint32_t *__restrict__ n_next) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    bool cont = false;  // (no early return: every lane takes part in the ballot)
    uint32_t j = i;
    float thr[3] = {1.f, 1.f, 1.f};
    f3 p2 = mk3(0, 0, 0), wi = mk3(0, 0, 1);
    if (i < n) {
        if (chain_in) {
            const float4 c = chain_in[i];
            thr[0] = c.x;
            thr[1] = c.y;
            thr[2] = c.z;
            j = __float_as_uint(c.w);
        }
        const uint4 h = hit[i];
        const int32_t prim = (int32_t)h.z;
        const float4 d4 = ray_d[i];
        const f3 rd = mk3(d4.x, d4.y, d4.z);
        if (prim < 0) {
            const f3 env = sample_env(S, rd);
            r0[j] = make_float4(thr[0] * env.x, thr[1] * env.y, thr[2] * env.z, __uint_as_float(kLitMiss));
            r1[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            r2[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const double t = hit_t(h);
            const uint32_t mat_bits = h.w;
            const float4 o4 = ray_o[i];
            const f3 ro = mk3(o4.x, o4.y, o4.z);
            const f3 p = ro + rd * (float)t;
            f3 nrm;
            f2 uv;
            hit_surface(S, prim, mat_bits, ro, rd, p, nrm, uv);
            const MaterialRec &M = S.mats[mat_bits & kMatIndexMask];
            cont = chain_continues(M, mat_bits, b, max_b);
            if (cont) {  // the bounce every chain pass takes (csrc/mcpt_chain.h)
                const f3 wo = -rd;
                chain_bounce(M, rd, p, nrm, p2, wi);
                if (M.type == MCPT_SMOOTH_CONDUCTOR || M.type == MCPT_ROUGH_CONDUCTOR)
                    for (int c = 0; c < 3; ++c) thr[c] *= mat_eval(M, wi, wo, nrm, c, uv, true);
            } else if (mat_bits >> 31) {  // Scene.cpp:102-107, at every chain depth
                const float cs = fabsf(dot(-rd, nrm));
                r0[j] = make_float4(thr[0] * clampf(0, 1, M.emit[0] * cs), thr[1] * clampf(0, 1, M.emit[1] * cs), thr[2] * clampf(0, 1, M.emit[2] * cs),
                                    __uint_as_float(kLitEmitter));
                r1[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                r2[j] = make_float4(p.x, p.y, p.z, 0.f);
            } else {
                float alb[3];
                hit_albedo(M, mat_bits, uv, alb);
                if (dot(nrm, rd) > 0) nrm = -nrm;
                r0[j] = make_float4(thr[0] * alb[0], thr[1] * alb[1], thr[2] * alb[2], __uint_as_float(kLitSurface));
                r1[j] = make_float4(nrm.x, nrm.y, nrm.z, 0.f);
                r2[j] = make_float4(p.x, p.y, p.z, 0.f);
            }
        }
    }
    const unsigned long long mask = __ballot(cont);
    if (mask == 0ull) return;
    uint32_t base = 0;
    if (lane_id() == 0) base = atomicAdd(n_next, (uint32_t)__popcll(mask));
    base = __shfl(base, 0);
    if (cont) {
        const uint32_t k = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        next_o[k] = make_float4(p2.x, p2.y, p2.z, 0.f);
        next_d[k] = make_float4(wi.x, wi.y, wi.z, 0.f);
        chain_out[k] = make_float4(thr[0], thr[1], thr[2], __uint_as_float(j));
    }
}

// One lane per sample of a chunk: the lookup of a sample that ended on a surface, r0[j].xyz = a * max(E, 0).  VIS: pd::shade_visible,
// else sh::probe_shade.  The surface samples of the launch are counted by ballot, one integer atomic per wave.
// DIRECT: the sampled direct term D of the sample waits in dd[j].xyz, and r0[j].xyz = a * (max(E, 0) + D).
template <bool VIS, bool DIRECT>
__global__ __launch_bounds__(kPbBlock) void k_lit_shade(sh::Grid g, const float *__restrict__ coef, const float *__restrict__ moments,
                                                      const int32_t *__restrict__ counts, float normal_bias, float backface_max, uint32_t n,
                                                      float4 *__restrict__ r0, const float4 *__restrict__ r1, const float4 *__restrict__ r2,
                                                      const float4 *__restrict__ dd, unsigned long long *__restrict__ lookups) {
    const uint32_t j = blockIdx.x * kPbBlock + threadIdx.x;
    bool surface = false;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n) {
        a = r0[j];
        surface = __float_as_uint(a.w) == kLitSurface;
    }
    if (surface) {
        const float4 n4 = r1[j], p4 = r2[j];
        const float p[3] = {p4.x, p4.y, p4.z}, nf[3] = {n4.x, n4.y, n4.z};
        float e[3];
        if (VIS) pd::shade_visible(g, coef, moments, counts, normal_bias, backface_max, p, nf, e, nullptr);
        else sh::probe_shade(g, coef, p, nf, e);
        if (DIRECT) {
            const float4 d = dd[j];
            r0[j] = make_float4(a.x * (fmaxf(e[0], 0.f) + d.x), a.y * (fmaxf(e[1], 0.f) + d.y), a.z * (fmaxf(e[2], 0.f) + d.z), a.w);
        } else {
            r0[j] = make_float4(a.x * fmaxf(e[0], 0.f), a.y * fmaxf(e[1], 0.f), a.z * fmaxf(e[2], 0.f), a.w);
        }
    }
    const unsigned long long mask = __ballot(surface);
    if (mask != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(lookups, (unsigned long long)__popcll(mask));
}

// One lane per pixel: the samples' values and hit points folded in sample order.
__global__ __launch_bounds__(kPbBlock) void k_lit_fold(uint32_t p0, uint32_t n_pix, int32_t aov_spp, const float4 *__restrict__ r0,
                                                     const float4 *__restrict__ r2, float *__restrict__ lit, float *__restrict__ position) {
    const uint32_t i = blockIdx.x * kPbBlock + threadIdx.x;
    if (i >= n_pix) return;
    const float fn = (float)aov_spp;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, q0 = 0.f, q1 = 0.f, q2 = 0.f;
    int32_t hits = 0;
    const size_t base = (size_t)i * aov_spp;
    for (int32_t k = 0; k < aov_spp; ++k) {
        const float4 v = r0[base + k];
        v0 += v.x / fn;
        v1 += v.y / fn;
        v2 += v.z / fn;
        if (__float_as_uint(v.w) != kLitMiss) {
            const float4 q = r2[base + k];
            q0 += q.x;
            q1 += q.y;
            q2 += q.z;
            ++hits;
        }
    }
    const size_t m = 3 * (size_t)(p0 + i);
    lit[m] = v0;
    lit[m + 1] = v1;
    lit[m + 2] = v2;
    if (position) {
        const float fh = (float)hits;
        position[m] = hits > 0 ? q0 / fh : 0.f;
        position[m + 1] = hits > 0 ? q1 / fh : 0.f;
        position[m + 2] = hits > 0 ? q2 / fh : 0.f;
    }
}

// The projection fold of mcpt_probe_volume_relight: one wave per probe, lane l < 27 owns coefficient j = l / 3 of channel c = l % 3 (the
// other lanes prepare samples and walk along, and store nothing).  Per block of 64 samples lane s prepares sample s: its value r0[g].xyz
// (0.f for an emitter with zero_emitters: the indirect_only flavour is consumed here, k_lit_terminal does not know it) and the nine
// weights of its staged direction ray_d[g].xyz.  Then the wave walks the block in sample order with the sample's three values and nine
// weights broadcast from lane s by wave-uniform lane reads; a lane picks its own with selects (an indexed w[j] would live in scratch) and
// adds to its sum in a register.  load: the sums continue what out holds (an earlier piece of the same probe's samples); last: these
// are the probes' last samples, so the blend with prev (the previous volume's coefficients, read only with h != 0) is applied.
__global__ __launch_bounds__(kPbBlock) void k_probe_relight_fold(const float4 *__restrict__ r0, const float4 *__restrict__ ray_d, uint32_t i0, uint32_t m,
                                                               uint32_t kc, int load, int last, int zero_emitters, float fn, float h,
                                                               const float *__restrict__ prev, float *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pi = blockIdx.x * (kPbBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pi >= m) return;  // (wave-uniform)
    const bool owner = lane < (uint32_t)sh::kRow;
    const uint32_t q = owner ? lane : 0u, j = q / 3u, c = q - 3u * j;
    const size_t row = ((size_t)i0 + pi) * (size_t)sh::kRow + q;
    float acc = 0.f;
    if (load) acc = out[row];
    const size_t base = (size_t)pi * kc;
    for (uint32_t kb = 0; kb < kc; kb += 64u) {
        const uint32_t cnt = kc - kb < 64u ? kc - kb : 64u;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, w[sh::kCoef];
#pragma unroll
        for (int32_t b = 0; b < sh::kCoef; ++b) w[b] = 0.f;
        if (lane < cnt) {
            const size_t g = base + kb + lane;
            const float4 r = r0[g], d4 = ray_d[g];
            const bool zero = zero_emitters && __float_as_uint(r.w) == kLitEmitter;
            v0 = zero ? 0.f : r.x;
            v1 = zero ? 0.f : r.y;
            v2 = zero ? 0.f : r.z;
            const float d[3] = {d4.x, d4.y, d4.z};
            float Y[sh::kCoef];
            sh::sh9_basis(d, Y);
#pragma unroll
            for (int32_t b = 0; b < sh::kCoef; ++b) w[b] = pr::weight(Y[b]);
        }
        for (uint32_t s = 0; s < cnt; ++s) {  // (a uniform bound: the tail of a short block is not walked)
            const float s0 = lane_read(v0, s), s1 = lane_read(v1, s), s2 = lane_read(v2, s);
            const float vs = c == 0u ? s0 : (c == 1u ? s1 : s2);
            float ws = lane_read(w[0], s);
#pragma unroll
            for (uint32_t b = 1; b < (uint32_t)sh::kCoef; ++b) {
                const float wb = lane_read(w[b], s);
                ws = j == b ? wb : ws;
            }
            acc = pr::fold_term(acc, vs, ws, fn);
        }
    }
    if (last) acc = pr::blend(h, h != 0.0f ? prev[row] : 0.f, acc);
    if (owner) out[row] = acc;
}

inline uint32_t probe_blocks(uint32_t n) { return (n + kPbBlock - 1) / kPbBlock; }

// The grid of a call, or the reason it is refused.
int check_grid(const std::string &w, const mcpt_probe_grid *grid, sh::Grid &g) {
    if (!grid) return fail(MCPT_ERR_ARG, w + ": null grid");
    if (grid->reserved[0] || grid->reserved[1] || grid->reserved[2]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    int64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = grid->origin[a];
        g.spacing[a] = grid->spacing[a];
        g.dims[a] = grid->dims[a];
        if (grid->dims[a] < 1) return fail(MCPT_ERR_ARG, w + ": every member of dims must be >= 1");
        if (!(grid->spacing[a] > 0.f) || !std::isfinite(grid->spacing[a])) return fail(MCPT_ERR_ARG, w + ": spacing must be positive and finite");
        n *= (int64_t)grid->dims[a];
        if (n > (int64_t)sh::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 27 probes");
    }
    return MCPT_OK;
}

int64_t grid_probes(const sh::Grid &g) { return (int64_t)g.dims[0] * g.dims[1] * g.dims[2]; }

// The refusals of mcpt_query_probes that depend on the parameters alone; mcpt_bake_probe_grid makes them before it touches the device.
int check_probe_params(const std::string &w, const mcpt_params &p, bool variance) {
    if (p.nranks > 1 || p.rank != 0) return fail(MCPT_ERR_ARG, w + ": nranks must be 1 and rank 0 (probes are not partitioned)");
    if (p.spp <= 0 || p.n_dir_sample <= 0 || !(p.rr_rate > 0.f)) return fail(MCPT_ERR_ARG, w + ": spp/n_dir_sample/rr_rate must be positive");
    if (variance && (p.spp < 2 || p.accumulate != 0 || p.spp_total != 0 || p.sample_offset != 0))
        return fail(MCPT_ERR_ARG, w + ": variance needs spp >= 2 and accumulate, spp_total and sample_offset 0");
    return MCPT_OK;
}

// A scene-owned buffer of at least n floats.  Enlarging frees the old allocation, which kernels of an earlier call enqueued on another
// stream may still be reading: wait on the host for the scene's last recorded query first.
hipError_t probe_grow(mcpt_scene *sc, DevBuf<float> &b, size_t n) {
    if (b.p && b.n >= n) return hipSuccess;
    const hipError_t e = query_settle(sc);
    if (e != hipSuccess) return e;
    sc->probes.allocations++;
    return b.alloc(n);
}

// The refusals of mcpt_query_probe_depth that depend on the parameters alone.
int check_depth_params(const std::string &w, const mcpt_probe_depth_params *p) {
    if (!p) return fail(MCPT_ERR_ARG, w + ": null depth params");
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    if (p->spp <= 0 || p->sample_offset < 0 || (int64_t)p->sample_offset + (int64_t)p->spp > 0x7fffffff)
        return fail(MCPT_ERR_ARG, w + ": spp must be positive, sample_offset >= 0 and sample_offset + spp at most 2^31 - 1 (the int32 counts)");
    if (p->accumulate != 0 && p->accumulate != 1) return fail(MCPT_ERR_ARG, w + ": accumulate must be 0 or 1");
    if (!(p->max_distance > 0.f) || !std::isfinite(p->max_distance)) return fail(MCPT_ERR_ARG, w + ": max_distance must be positive and finite");
    return MCPT_OK;
}

// The options of the _ex probe calls (nullable: every switch off).
int check_probe_opts(const std::string &w, const mcpt_probe_opts *o, bool &indirect_only) {
    indirect_only = false;
    if (!o) return MCPT_OK;
    if (o->indirect_only != 0 && o->indirect_only != 1) return fail(MCPT_ERR_ARG, w + ": indirect_only must be 0 or 1");
    for (int k = 0; k < 7; ++k)
        if (o->reserved[k]) return fail(MCPT_ERR_ARG, w + ": reserved words of the probe options must be 0");
    indirect_only = o->indirect_only == 1;
    return MCPT_OK;
}

int check_visibility(const std::string &w, const mcpt_probe_visibility *o) {
    if (!o) return fail(MCPT_ERR_ARG, w + ": null visibility options");
    if (o->reserved[0] || o->reserved[1]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    if (!(o->normal_bias >= 0.f) || !std::isfinite(o->normal_bias) || !(o->backface_max >= 0.f) || !std::isfinite(o->backface_max))
        return fail(MCPT_ERR_ARG, w + ": normal_bias and backface_max must be finite and not negative");
    return MCPT_OK;
}

// Whether the byte ranges [a, a + na) and [b, b + nb) share a byte.
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// A scene-owned buffer of mcpt_probe_volume_relight of at least n entries; grown behind query_settle, like probe_grow.
template <class T>
hipError_t relit_grow(mcpt_scene *sc, DevBuf<T> &b, size_t n, mcpt_query_info &qi) {
    if (b.p && b.n >= n) return hipSuccess;
    const hipError_t e = query_settle(sc);
    if (e != hipSuccess) return e;
    sc->probes.allocations++;
    qi.grew = 1;
    return b.alloc(n);
}

}  // namespace

void launch_lit_terminal(const DevScene &S, uint32_t n, int32_t b, int32_t max_b, const float4 *ray_o, const float4 *ray_d, const uint4 *hit,
                         const float4 *chain_in, float4 *r0, float4 *r1, float4 *r2, float4 *next_o, float4 *next_d, float4 *chain_out,
                         uint32_t *n_next, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_lit_terminal, dim3(probe_blocks(n)), dim3(kPbBlock), 0, st, S, n, b, max_b, ray_o, ray_d, hit, chain_in, r0, r1, r2, next_o, next_d,
                       chain_out, n_next);
}

void launch_lit_shade(const LitVolume &vol, uint32_t n, float4 *r0, const float4 *r1, const float4 *r2, const float4 *direct_d, unsigned long long *lookups,
                      hipStream_t st) {
    if (n == 0) return;
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(probe_blocks(n)), dim3(kPbBlock), 0, st, vol.g, vol.sh, vol.moments, vol.counts, vol.normal_bias, vol.backface_max, n, r0,
                           r1, r2, direct_d, lookups);
    };
    if (vol.moments) direct_d ? go(k_lit_shade<true, true>) : go(k_lit_shade<true, false>);
    else direct_d ? go(k_lit_shade<false, true>) : go(k_lit_shade<false, false>);
}

int direct_term(const DevScene &S, DirectRays src, uint64_t n, const DirectStage &stg, float *out, uint32_t stride, hipStream_t st, int32_t &pieces) {
    // Where a point's samples take several pieces (piece_cut, csrc/mcpt_direct.h) its sum passes through `out` between launches; either way
    // a point's additions run in sample order.
    src.ray_o = stg.ray_o;
    src.ray_d = stg.ray_d;
    src.slot = stg.slot;
    src.n_rays = stg.n_rays;
    return for_each_piece(stg.cut, n, (uint64_t)src.N, [&](uint32_t i0, uint32_t m, uint32_t j0, uint32_t jc) -> int {
        src.i0 = i0;
        src.m = m;
        src.j0 = j0;
        src.jc = jc;
        HIP_TRY(hipMemsetAsync(stg.n_rays, 0, sizeof(uint32_t), st));
        launch_direct_rays(S, src, st);
        launch_trace_closest(S, m * jc, stg.n_rays, stg.ray_o, stg.ray_d, stg.hit, stg.rl, st);
        hipLaunchKernelGGL(k_direct_fold, dim3(probe_blocks(m)), dim3(kPbBlock), 0, st, i0, m, jc, j0 > 0 ? 1 : 0, j0 + jc == (uint32_t)src.N ? 1 : 0,
                           stg.slot, stg.ray_d, stg.hit, out, stride);
        pieces++;
        return MCPT_OK;
    });
}

void launch_lit_fold(uint32_t p0, uint32_t n_pix, int32_t aov_spp, const float4 *r0, const float4 *r2, float *lit, float *position, hipStream_t st) {
    if (n_pix == 0) return;
    hipLaunchKernelGGL(k_lit_fold, dim3(probe_blocks(n_pix)), dim3(kPbBlock), 0, st, p0, n_pix, aov_spp, r0, r2, lit, position);
}

}  // namespace mcpt

// mcpt_render_probe_lit and mcpt_render_probe_lit_direct after the former has cleared its info: every refusal, then the pass.
static int render_probe_lit(const std::string &w, mcpt_scene *sc, const mcpt_camera *cam, const mcpt_lit_opts *opts, const mcpt_lit_direct_opts *direct,
                            const mcpt_probe_volume *vol, const mcpt_lit_outputs *out, void *hip_stream, mcpt_lit_info *info, mcpt_lit_direct_info *dinfo) {
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, w + ": " + what); };
    if (!sc || !cam || !opts || !vol || !out) return bad("null scene, camera, opts, volume or outputs");
    if (!out->lit || !vol->sh) return bad("null lit or sh");
    if (opts->aov_spp < 0 || opts->aov_spp > kMaxAovSpp) return bad("aov_spp must be 0..65536");
    if (opts->specular_depth < 0 || opts->specular_depth > dn::kMaxSpecularDepth) return bad("specular_depth must be 0..8");
    if (opts->centre != 0 && opts->centre != 1) return bad("centre must be 0 or 1");
    if (opts->reserved[0] || opts->reserved[1] || opts->reserved[2] || opts->reserved[3] || out->reserved[0] || out->reserved[1])
        return bad("reserved words and pointers must be 0");
    if (opts->centre == 1 && opts->aov_spp > 1) return bad("centre 1 takes one ray per pixel (aov_spp must be 0 or 1)");
    if (direct) {
        if (direct->n_samples < 0 || direct->n_samples > dl::kMaxSamples) return bad("direct: n_samples must be 0 (off) or 1 .. 4096");
        for (int k = 0; k < 6; ++k)
            if (direct->reserved[k]) return bad("direct: reserved words must be 0");
    }
    const bool vis = vol->moments != nullptr;
    if ((vol->counts != nullptr) != vis || (vol->visibility != nullptr) != vis) return bad("moments, counts and visibility must be all null or all non-null");
    if (!frame_ok(cam->width, cam->height)) return bad("width and height must be positive (and the frame not too large)");
    LitVolume lv;
    const int gc = check_grid(w, vol->grid, lv.g);
    if (gc != MCPT_OK) return gc;
    if (vis) {
        if (grid_probes(lv.g) > (int64_t)pd::kMaxProbes) return bad("dims must name at most (2^31 - 1) / 192 probes");
        const int vc = check_visibility(w, vol->visibility);
        if (vc != MCPT_OK) return vc;
        lv.normal_bias = vol->visibility->normal_bias;
        lv.backface_max = vol->visibility->backface_max;
    }
    lv.sh = vol->sh;
    lv.moments = vol->moments;
    lv.counts = vol->counts;
    if (!on_device(out->lit, sc->device) || !on_device(vol->sh, sc->device) || (out->position && !on_device(out->position, sc->device)) ||
        (vis && (!on_device(vol->moments, sc->device) || !on_device(vol->counts, sc->device))))
        return bad("lit, position, sh, moments and counts must be memory of the scene's device");
    const Clock::time_point t0 = Clock::now();
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    if (!sc->probes.lit_count.p) HIP_TRY(sc->probes.lit_count.alloc(2));  // {lookups, live light samples}
    mcpt_lit_info li;
    std::memset(&li, 0, sizeof li);
    mcpt_lit_direct_info di;
    std::memset(&di, 0, sizeof di);
    const int32_t n_spp = opts->aov_spp == 0 ? 1 : opts->aov_spp;
    const LitDirect ld{direct ? direct->n_samples : 0, direct ? direct->seed : 0u};
    const int rc = lit_pass(sc, make_camera(*cam), opts->seed, n_spp, opts->specular_depth, opts->centre == 1, lv, out->lit, out->position,
                            sc->probes.lit_count.p, (hipStream_t)hip_stream, li, ld.n_samples > 0 ? &ld : nullptr, &di);
    if (rc != MCPT_OK) return drained(rc);
    li.ms_total = ms_since(t0);
    if (info) *info = li;
    if (dinfo) *dinfo = di;
    return MCPT_OK;
}

extern "C" {

int mcpt_render_probe_lit(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_lit_opts *opts, const mcpt_probe_volume *vol, const mcpt_lit_outputs *out,
                          void *hip_stream, mcpt_lit_info *info) {
    if (info) std::memset(info, 0, sizeof *info);
    return render_probe_lit("mcpt_render_probe_lit", sc, cam, opts, nullptr, vol, out, hip_stream, info, nullptr);
}

int mcpt_render_probe_lit_direct(mcpt_scene *sc, const mcpt_camera *cam, const mcpt_lit_opts *opts, const mcpt_lit_direct_opts *direct,
                                 const mcpt_probe_volume *vol, const mcpt_lit_outputs *out, void *hip_stream, mcpt_lit_info *info,
                                 mcpt_lit_direct_info *dinfo) {
    return render_probe_lit("mcpt_render_probe_lit_direct", sc, cam, opts, direct, vol, out, hip_stream, info, dinfo);
}

int mcpt_query_probes(mcpt_scene *sc, const mcpt_params *pp, int64_t n, const float *origins, const mcpt_probe_outputs *out, void *hip_stream,
                      mcpt_stats *stats) {
    return mcpt_query_probes_ex(sc, pp, n, origins, out, hip_stream, stats, nullptr);
}

int mcpt_query_probes_ex(mcpt_scene *sc, const mcpt_params *pp, int64_t n, const float *origins, const mcpt_probe_outputs *out, void *hip_stream,
                         mcpt_stats *stats, const mcpt_probe_opts *opts) {
    const auto bad = [](const char *what) { return fail(MCPT_ERR_ARG, std::string("mcpt_query_probes: ") + what); };
    if (!sc) return bad("null scene");
    bool indirect_only = false;
    const int oc = check_probe_opts("mcpt_query_probes", opts, indirect_only);
    if (oc != MCPT_OK) return oc;
    if (!pp || !out) return bad("null params or out");
    const mcpt_params &p = *pp;
    if (n < 0 || n > (int64_t)sh::kMaxProbes) return bad("n must be in 0 .. (2^31 - 1) / 27");
    if (out->reserved) return bad("the reserved word must be null");
    const int pc = check_probe_params("mcpt_query_probes", p, out->variance != nullptr);
    if (pc != MCPT_OK) return pc;
    if (n == 0) {
        if (stats) std::memset(stats, 0, sizeof *stats);
        return MCPT_OK;
    }
    if (!origins || !out->sh) return bad("null origins or sh");
    if (!on_device(origins, sc->device) || !on_device(out->sh, sc->device) || (out->radiance && !on_device(out->radiance, sc->device)) ||
        (out->variance && !on_device(out->variance, sc->device)))
        return bad("origins, sh, radiance and variance must be memory of the scene's device");
    float *radiance = out->radiance;
    if (!radiance) {  // the plain fold still runs: the scene's own buffer takes its place (with accumulate its content means nothing)
        HIP_TRY(hipSetDevice(sc->device));
        HIP_TRY(probe_grow(sc, sc->probes.radiance, (size_t)n * 3));
        radiance = sc->probes.radiance.p;
    }
    return sensor_radiance(sc, p, (uint32_t)n, SensorConst{origins, nullptr, kSensorSphere, indirect_only ? 1 : 0}, radiance, out->variance, out->sh,
                           (hipStream_t)hip_stream, stats);
}

int mcpt_probe_rays(mcpt_scene *sc, uint32_t seed, int64_t n, const float *origins, const uint32_t *sensor, const uint32_t *sample, float *origins_out,
                    float *dirs_out) {
    if (!sc || n < 0 || (n > 0 && (!origins || !sensor || !sample || !origins_out || !dirs_out))) return fail(MCPT_ERR_ARG, "mcpt_probe_rays: bad argument");
    if (n == 0) return MCPT_OK;
    if (n > 0x7fffffff) return fail(MCPT_ERR_ARG, "mcpt_probe_rays: too many rays for one call");
    size_t m = 0;  // the probes the pairs name: rows 0 .. max(sensor) of origins
    for (int64_t j = 0; j < n; ++j) m = std::max<size_t>(m, (size_t)sensor[j] + 1);
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf<float> dPo;
    DevBuf<uint32_t> dI, dS;
    DevBuf<float4> dO, dD;
    HIP_TRY(dO.alloc(n));
    HIP_TRY(dD.alloc(n));
    HIP_TRY(upload(dPo, origins, m * 3));
    HIP_TRY(upload(dI, sensor, n));
    HIP_TRY(upload(dS, sample, n));
    launch_sensor_rays(SensorConst{dPo.p, nullptr, kSensorSphere}, seed, (uint32_t)n, dI.p, dS.p, dO.p, dD.p, nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<float4> o(n), d(n);
    HIP_TRY(download(o.data(), dO, n));
    HIP_TRY(download(d.data(), dD, n));
    for (int64_t j = 0; j < n; ++j) {
        origins_out[3 * j] = o[j].x, origins_out[3 * j + 1] = o[j].y, origins_out[3 * j + 2] = o[j].z;
        dirs_out[3 * j] = d[j].x, dirs_out[3 * j + 1] = d[j].y, dirs_out[3 * j + 2] = d[j].z;
    }
    return MCPT_OK;
}

int mcpt_probe_shade(mcpt_scene *sc, const mcpt_probe_grid *grid, const float *coef, int64_t n, const float *points, const float *normals, float *out,
                     void *hip_stream) {
    const std::string w = "mcpt_probe_shade";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (n < 0 || n > 0x7fffffff / 3) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 3");
    if (n == 0) return MCPT_OK;
    if (!coef || !points || !normals || !out) return fail(MCPT_ERR_ARG, w + ": null sh, points, normals or out");
    if (!on_device(coef, sc->device) || !on_device(points, sc->device) || !on_device(normals, sc->device) || !on_device(out, sc->device))
        return fail(MCPT_ERR_ARG, w + ": sh, points, normals and out must be memory of the scene's device");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_probe_shade, dim3(probe_blocks((uint32_t)n)), dim3(kPbBlock), 0, (hipStream_t)hip_stream, g, coef, (uint32_t)n, points, normals, out);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_bake_probe_grid(mcpt_scene *sc, const mcpt_probe_grid *grid, const mcpt_params *pp, float *coef, void *hip_stream, mcpt_stats *stats) {
    return mcpt_bake_probe_grid_ex(sc, grid, pp, coef, hip_stream, stats, nullptr);
}

int mcpt_bake_probe_grid_ex(mcpt_scene *sc, const mcpt_probe_grid *grid, const mcpt_params *pp, float *coef, void *hip_stream, mcpt_stats *stats,
                            const mcpt_probe_opts *opts) {
    const std::string w = "mcpt_bake_probe_grid";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    bool indirect_only = false;
    const int oc = check_probe_opts(w, opts, indirect_only);
    if (oc != MCPT_OK) return oc;
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (!pp || !coef) return fail(MCPT_ERR_ARG, w + ": null params or sh");
    const int pc = check_probe_params(w, *pp, false);
    if (pc != MCPT_OK) return pc;
    if (!on_device(coef, sc->device)) return fail(MCPT_ERR_ARG, w + ": sh must be memory of the scene's device");
    const uint32_t n = (uint32_t)grid_probes(g);
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    HIP_TRY(probe_grow(sc, sc->probes.points, (size_t)n * 3));
    hipLaunchKernelGGL(k_probe_grid_points, dim3(probe_blocks(n)), dim3(kPbBlock), 0, (hipStream_t)hip_stream, g, n, sc->probes.points.p);
    HIP_TRY(hipGetLastError());
    const mcpt_probe_outputs out{coef, nullptr, nullptr, nullptr};
    return mcpt_query_probes_ex(sc, pp, n, sc->probes.points.p, &out, hip_stream, stats, opts);
}

int mcpt_query_probe_depth(mcpt_scene *sc, const mcpt_probe_depth_params *pp, int64_t n, const float *origins, float *moments, int32_t *counts,
                           void *hip_stream, mcpt_query_info *info) {
    const std::string w = "mcpt_query_probe_depth";
    if (info) std::memset(info, 0, sizeof *info);
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    const int pc = check_depth_params(w, pp);
    if (pc != MCPT_OK) return pc;
    if (n < 0 || n > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 192");
    if (n == 0) return MCPT_OK;
    if (!origins || !moments || !counts) return fail(MCPT_ERR_ARG, w + ": null origins, moments or counts");
    if (!on_device(origins, sc->device) || !on_device(moments, sc->device) || !on_device(counts, sc->device))
        return fail(MCPT_ERR_ARG, w + ": origins, moments and counts must be memory of the scene's device");
    const mcpt_probe_depth_params &p = *pp;
    const hipStream_t st = (hipStream_t)hip_stream;
    mcpt_query_info qi;
    std::memset(&qi, 0, sizeof qi);
    HIP_TRY(hipSetDevice(sc->device));
    // A launch holds whole probes when a probe's samples fit the staging (their sums never leave the registers), else whole 64-sample blocks
    // of one probe (the sums pass through `moments` between launches).  Either way a texel's additions run in sample order.
    const PieceCut cut = piece_cut((uint64_t)n, (uint64_t)p.spp, std::max<uint32_t>(sc->knobs.query_chunk, 64u), 64);
    RetryList rl;
    const int sr = query_stage(sc, (uint32_t)cut.staged(), st, qi, rl);
    if (sr != MCPT_OK) return sr;
    QueryBufs &Q = sc->query;
    for_each_piece(cut, (uint64_t)n, (uint64_t)p.spp, [&](uint32_t i0, uint32_t m, uint32_t k0, uint32_t kc) -> int {
        const uint32_t rays = m * kc;
        hipLaunchKernelGGL(k_probe_depth_rays, dim3(probe_blocks(rays)), dim3(kPbBlock), 0, st, origins, p.seed, i0, kc, (uint32_t)p.sample_offset + k0, rays,
                           Q.ray_o.p, Q.ray_d.p);
        launch_trace_closest(sc->view, rays, nullptr, Q.ray_o.p, Q.ray_d.p, Q.hit.p, rl, st);
        hipLaunchKernelGGL(k_probe_depth_fold, dim3((m + kPbBlock / 64 - 1) / (kPbBlock / 64)), dim3(kPbBlock), 0, st, sc->view, Q.ray_o.p, Q.ray_d.p, Q.hit.p,
                           i0, m, kc, (p.accumulate || k0 > 0) ? 1 : 0, p.max_distance, moments, counts);
        qi.launches++;
        return MCPT_OK;
    });
    const int fr = query_finish(sc, st, qi);
    if (fr != MCPT_OK) return fr;
    if (info) *info = qi;
    return MCPT_OK;
}

int mcpt_query_direct(mcpt_scene *sc, const mcpt_direct_opts *op, int64_t n, const float *points, const float *normals, float *out, void *hip_stream,
                      mcpt_query_info *info) {
    const std::string w = "mcpt_query_direct";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    if (!op) return fail(MCPT_ERR_ARG, w + ": null opts");
    if (op->n_samples < 1 || op->n_samples > dl::kMaxSamples) return fail(MCPT_ERR_ARG, w + ": n_samples must be in 1 .. 4096");
    for (int k = 0; k < 5; ++k)
        if (op->reserved[k]) return fail(MCPT_ERR_ARG, w + ": reserved words must be 0");
    if (n < 0 || n > (int64_t)0x7fffffff / op->n_samples) return fail(MCPT_ERR_ARG, w + ": n must not be negative and n * n_samples at most 2^31 - 1");
    if (n > 0 && (!points || !normals || !out)) return fail(MCPT_ERR_ARG, w + ": null points, normals or out");
    if (n > 0 && (!on_device(points, sc->device) || !on_device(normals, sc->device) || !on_device(out, sc->device)))
        return fail(MCPT_ERR_ARG, w + ": points, normals and out must be memory of the scene's device");
    if (info) std::memset(info, 0, sizeof *info);
    if (n == 0) return MCPT_OK;
    const hipStream_t st = (hipStream_t)hip_stream;
    mcpt_query_info qi;
    std::memset(&qi, 0, sizeof qi);
    HIP_TRY(hipSetDevice(sc->device));
    const PieceCut cut = piece_cut((uint64_t)n, (uint64_t)op->n_samples, std::max<uint32_t>(sc->knobs.query_chunk, 64u), 1);
    const bool lit = sc->view.n_lights > 0;  // (an empty light table: exact zeros, no ray)
    RetryList rl;
    const int sr = query_stage(sc, lit ? (uint32_t)cut.staged() : 1u, st, qi, rl);
    if (sr != MCPT_OK) return sr;
    QueryBufs &Q = sc->query;
    if (!lit) {
        HIP_TRY(hipMemsetAsync(out, 0, (size_t)n * 3 * sizeof(float), st));
        qi.launches = 1;
    } else {
        if (Q.direct_slot.n < cut.staged() || !Q.direct_n.p) {
            HIP_TRY(query_settle(sc));
            HIP_TRY(Q.direct_slot.alloc(cut.staged()));
            HIP_TRY(Q.direct_n.alloc(1));
            qi.grew = 1;
        }
        DirectRays src{};
        src.points = points;
        src.normals = normals;
        src.seed = op->seed;
        src.key_sample = op->key_sample;
        src.N = op->n_samples;
        const int dr = direct_term(sc->view, src, (uint64_t)n, DirectStage{Q.ray_o.p, Q.ray_d.p, Q.direct_slot.p, Q.hit.p, Q.direct_n.p, cut, rl}, out, 3u, st, qi.launches);
        if (dr != MCPT_OK) return dr;
    }
    const int fr = query_finish(sc, st, qi);
    if (fr != MCPT_OK) return fr;
    qi.staged_bytes += (int64_t)(Q.direct_slot.bytes() + Q.direct_n.bytes());
    if (info) *info = qi;
    return MCPT_OK;
}

int mcpt_probe_volume_relight(mcpt_scene *sc, const mcpt_probe_volume *vol, const mcpt_probe_relight_opts *op, const mcpt_probe_relight_outputs *out,
                              void *hip_stream, mcpt_query_info *info) {
    const std::string w = "mcpt_probe_volume_relight";
    const auto bad = [&](const char *what) { return fail(MCPT_ERR_ARG, w + ": " + what); };
    if (!sc || !vol || !op || !out) return bad("null scene, volume, opts or outputs");
    if (!out->sh || !vol->sh) return bad("null sh");
    if (op->spp < 1 || op->sample_offset < 0 || (int64_t)op->sample_offset + (int64_t)op->spp > 0x7fffffff)
        return bad("spp must be positive, sample_offset >= 0 and sample_offset + spp at most 2^31 - 1");
    if (!(op->hysteresis >= 0.f) || !(op->hysteresis < 1.f)) return bad("hysteresis must be in [0, 1)");
    if (op->indirect_only != 0 && op->indirect_only != 1) return bad("indirect_only must be 0 or 1");
    if (op->direct_samples < 0 || op->direct_samples > dl::kMaxSamples) return bad("direct_samples must be 0 (off) or 1 .. 4096");
    for (int k = 0; k < 8; ++k)
        if (op->reserved[k]) return bad("reserved words must be 0");
    if (out->reserved) return bad("the reserved pointer must be null");
    const bool depth = out->moments != nullptr;
    if ((out->counts != nullptr) != depth) return bad("the outputs moments and counts must be both null or both non-null");
    if (depth && (!(op->max_distance > 0.f) || !std::isfinite(op->max_distance))) return bad("max_distance must be positive and finite when depth outputs are given");
    const bool vis = vol->moments != nullptr;
    if ((vol->counts != nullptr) != vis || (vol->visibility != nullptr) != vis) return bad("moments, counts and visibility must be all null or all non-null");
    LitVolume lv;
    const int gc = check_grid(w, vol->grid, lv.g);
    if (gc != MCPT_OK) return gc;
    const int64_t n = grid_probes(lv.g);
    if ((vis || depth) && n > (int64_t)pd::kMaxProbes) return bad("dims must name at most (2^31 - 1) / 192 probes");
    if (vis) {
        const int vc = check_visibility(w, vol->visibility);
        if (vc != MCPT_OK) return vc;
        lv.normal_bias = vol->visibility->normal_bias;
        lv.backface_max = vol->visibility->backface_max;
    }
    if (n > (int64_t)0x7fffffff / op->spp) return bad("probes * spp must be at most 2^31 - 1");
    if (op->direct_samples > 0 && n * op->spp > (int64_t)0x7fffffff / op->direct_samples) return bad("probes * spp * direct_samples must be at most 2^31 - 1");
    const size_t sh_bytes = (size_t)n * sh::kRow * sizeof(float), mom_bytes = (size_t)n * pd::kTexels * 3 * sizeof(float), cnt_bytes = (size_t)n * 2 * sizeof(int32_t);
    if (ranges_overlap(out->sh, sh_bytes, vol->sh, sh_bytes)) return bad("the output sh must not overlap the volume's sh");
    if (depth && vis && (ranges_overlap(out->moments, mom_bytes, vol->moments, mom_bytes) || ranges_overlap(out->counts, cnt_bytes, vol->counts, cnt_bytes)))
        return bad("the output moments and counts must not overlap the volume's");
    lv.sh = vol->sh;
    lv.moments = vol->moments;
    lv.counts = vol->counts;
    if (!on_device(out->sh, sc->device) || !on_device(vol->sh, sc->device) || (depth && (!on_device(out->moments, sc->device) || !on_device(out->counts, sc->device))) ||
        (vis && (!on_device(vol->moments, sc->device) || !on_device(vol->counts, sc->device))))
        return bad("sh, moments and counts of the volume and of the outputs must be memory of the scene's device");
    const hipStream_t st = (hipStream_t)hip_stream;
    mcpt_query_info qi;
    std::memset(&qi, 0, sizeof qi);
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    ProbeBufs &P = sc->probes;
    const int32_t N = sc->view.n_lights > 0 ? op->direct_samples : 0;  // (an empty light table: D = 0, no ray)
    const uint32_t cap = std::max<uint32_t>(sc->knobs.query_chunk, 64u);
    // the probe rays are cut as mcpt_query_probe_depth cuts them; the light samples of a piece's records as the lit pass cuts a chunk's
    const PieceCut cut = piece_cut((uint64_t)n, (uint64_t)op->spp, cap, 64);
    const uint64_t rec = cut.staged();
    const PieceCut dcut = piece_cut(rec, (uint64_t)std::max(N, 1), cap, 1);
    HIP_TRY(probe_grow(sc, P.points, (size_t)n * 3));
    HIP_TRY(relit_grow(sc, P.relit_r0, rec, qi));
    HIP_TRY(relit_grow(sc, P.relit_r1, rec, qi));
    HIP_TRY(relit_grow(sc, P.relit_r2, rec, qi));
    HIP_TRY(relit_grow(sc, P.relit_count, 1, qi));
    if (op->direct_samples > 0) HIP_TRY(relit_grow(sc, P.relit_d, rec, qi));
    if (N > 0) {
        HIP_TRY(relit_grow(sc, P.relit_ray_o, dcut.staged(), qi));
        HIP_TRY(relit_grow(sc, P.relit_ray_d, dcut.staged(), qi));
        HIP_TRY(relit_grow(sc, P.relit_slot, dcut.staged(), qi));
        HIP_TRY(relit_grow(sc, P.relit_hit, dcut.staged(), qi));
        HIP_TRY(relit_grow(sc, P.relit_n, 1, qi));
    }
    RetryList rl;
    const int sr = query_stage(sc, (uint32_t)std::max<uint64_t>(rec, N > 0 ? dcut.staged() : 0), st, qi, rl);
    if (sr != MCPT_OK) return sr;
    QueryBufs &Q = sc->query;
    HIP_TRY(hipMemsetAsync(P.relit_count.p, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_probe_grid_points, dim3(probe_blocks((uint32_t)n)), dim3(kPbBlock), 0, st, lv.g, (uint32_t)n, P.points.p);
    const float fn = (float)op->spp;
    const int rc = for_each_piece(cut, (uint64_t)n, (uint64_t)op->spp, [&](uint32_t i0, uint32_t m, uint32_t k0, uint32_t kc) -> int {
        const uint32_t rays = m * kc;
        const uint32_t first = (uint32_t)op->sample_offset + k0;
        const int load = k0 > 0 ? 1 : 0, last = k0 + kc == (uint32_t)op->spp ? 1 : 0;
        hipLaunchKernelGGL(k_probe_depth_rays, dim3(probe_blocks(rays)), dim3(kPbBlock), 0, st, P.points.p, op->seed, i0, kc, first, rays, Q.ray_o.p, Q.ray_d.p);
        launch_trace_closest(sc->view, rays, nullptr, Q.ray_o.p, Q.ray_d.p, Q.hit.p, rl, st);
        launch_lit_terminal(sc->view, rays, 0, 0, Q.ray_o.p, Q.ray_d.p, Q.hit.p, nullptr, P.relit_r0.p, P.relit_r1.p, P.relit_r2.p, nullptr, nullptr, nullptr, nullptr, st);
        float4 *direct_d = nullptr;
        if (op->direct_samples > 0) {
            direct_d = P.relit_d.p;
            if (N == 0) {
                HIP_TRY(hipMemsetAsync(direct_d, 0, (size_t)rays * sizeof(float4), st));
            } else {
                DirectRays src{};
                src.seed = op->direct_seed;
                src.N = N;
                src.r0 = P.relit_r0.p;
                src.r1 = P.relit_r1.p;
                src.r2 = P.relit_r2.p;
                src.surface_kind = kLitSurfaceKind;
                src.p0 = i0;  // record g of the piece is sample first + g % kc of probe i0 + g / kc
                src.aov_spp = (int32_t)kc;
                src.sample0 = first;
                const int dr = direct_term(sc->view, src, rays, DirectStage{P.relit_ray_o.p, P.relit_ray_d.p, P.relit_slot.p, P.relit_hit.p, P.relit_n.p, dcut, rl},
                                           reinterpret_cast<float *>(direct_d), 4u, st, qi.launches);
                if (dr != MCPT_OK) return dr;
            }
        }
        launch_lit_shade(lv, rays, P.relit_r0.p, P.relit_r1.p, P.relit_r2.p, direct_d, P.relit_count.p, st);
        const dim3 waves((m + kPbBlock / 64 - 1) / (kPbBlock / 64));
        hipLaunchKernelGGL(k_probe_relight_fold, waves, dim3(kPbBlock), 0, st, P.relit_r0.p, Q.ray_d.p, i0, m, kc, load, last, op->indirect_only, fn, op->hysteresis,
                           vol->sh, out->sh);
        if (depth)
            hipLaunchKernelGGL(k_probe_depth_fold, waves, dim3(kPbBlock), 0, st, sc->view, Q.ray_o.p, Q.ray_d.p, Q.hit.p, i0, m, kc, load, op->max_distance,
                               out->moments, out->counts);
        qi.launches++;
        return MCPT_OK;
    });
    const int fr = query_finish(sc, st, qi);  // (behind whatever was enqueued, also when a piece failed)
    if (rc != MCPT_OK) return rc;
    if (fr != MCPT_OK) return fr;
    qi.staged_bytes += (int64_t)(P.relit_r0.bytes() + P.relit_r1.bytes() + P.relit_r2.bytes() + P.relit_d.bytes() + P.relit_ray_o.bytes() + P.relit_ray_d.bytes() +
                                 P.relit_slot.bytes() + P.relit_hit.bytes() + P.relit_n.bytes());
    if (info) *info = qi;
    return MCPT_OK;
}

int mcpt_probe_relight_fold_host(int64_t n, int32_t spp, const float *dirs, const float *values, float hysteresis, const float *prev, float *out) {
    const std::string w = "mcpt_probe_relight_fold_host";
    if (n < 0 || n > (int64_t)sh::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 27");
    if (spp < 1) return fail(MCPT_ERR_ARG, w + ": spp must be positive");
    if (!(hysteresis >= 0.f) || !(hysteresis < 1.f)) return fail(MCPT_ERR_ARG, w + ": hysteresis must be in [0, 1)");
    if (n > 0 && (!dirs || !values || !out || (hysteresis != 0.f && !prev))) return fail(MCPT_ERR_ARG, w + ": null dirs, values or out, or null prev with a hysteresis");
    pr::fold_host(n, spp, dirs, values, hysteresis, prev, out);
    return MCPT_OK;
}

int mcpt_probe_shade_visible(mcpt_scene *sc, const mcpt_probe_grid *grid, const float *coef, const float *moments, const int32_t *counts,
                             const mcpt_probe_visibility *opts, int64_t n, const float *points, const float *normals, float *out, float *weight_out,
                             void *hip_stream) {
    const std::string w = "mcpt_probe_shade_visible";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (grid_probes(g) > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 192 probes");
    const int vc = check_visibility(w, opts);
    if (vc != MCPT_OK) return vc;
    if (n < 0 || n > 0x7fffffff / 3) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 3");
    if (n == 0) return MCPT_OK;
    if (!coef || !moments || !counts || !points || !normals || !out) return fail(MCPT_ERR_ARG, w + ": null sh, moments, counts, points, normals or out");
    if (!on_device(coef, sc->device) || !on_device(moments, sc->device) || !on_device(counts, sc->device) || !on_device(points, sc->device) ||
        !on_device(normals, sc->device) || !on_device(out, sc->device) || (weight_out && !on_device(weight_out, sc->device)))
        return fail(MCPT_ERR_ARG, w + ": sh, moments, counts, points, normals, out and weight_out must be memory of the scene's device");
    HIP_TRY(hipSetDevice(sc->device));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_probe_shade_visible, dim3(probe_blocks((uint32_t)n)), dim3(kPbBlock), 0, (hipStream_t)hip_stream, g, coef, moments, counts,
                       opts->normal_bias, opts->backface_max, (uint32_t)n, points, normals, out, weight_out);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_bake_probe_volume(mcpt_scene *sc, const mcpt_probe_grid *grid, const mcpt_params *pp, const mcpt_probe_depth_params *dp, float *coef,
                           float *moments, int32_t *counts, void *hip_stream, mcpt_stats *stats) {
    return mcpt_bake_probe_volume_ex(sc, grid, pp, dp, coef, moments, counts, hip_stream, stats, nullptr);
}

int mcpt_bake_probe_volume_ex(mcpt_scene *sc, const mcpt_probe_grid *grid, const mcpt_params *pp, const mcpt_probe_depth_params *dp, float *coef,
                              float *moments, int32_t *counts, void *hip_stream, mcpt_stats *stats, const mcpt_probe_opts *opts) {
    const std::string w = "mcpt_bake_probe_volume";
    if (!sc) return fail(MCPT_ERR_ARG, w + ": null scene");
    bool indirect_only = false;
    const int oc = check_probe_opts(w, opts, indirect_only);
    if (oc != MCPT_OK) return oc;
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (grid_probes(g) > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 192 probes");
    if (!pp || !coef || !moments || !counts) return fail(MCPT_ERR_ARG, w + ": null params, sh, moments or counts");
    const int pc = check_probe_params(w, *pp, false);
    if (pc != MCPT_OK) return pc;
    const int dc = check_depth_params(w, dp);
    if (dc != MCPT_OK) return dc;
    if (!on_device(coef, sc->device) || !on_device(moments, sc->device) || !on_device(counts, sc->device))
        return fail(MCPT_ERR_ARG, w + ": sh, moments and counts must be memory of the scene's device");
    const int rc = mcpt_bake_probe_grid_ex(sc, grid, pp, coef, hip_stream, stats, opts);
    if (rc != MCPT_OK) return rc;
    return mcpt_query_probe_depth(sc, dp, grid_probes(g), sc->probes.points.p, moments, counts, hip_stream, nullptr);
}

int mcpt_scene_probe_buffers(const mcpt_scene *sc, int64_t *floats, int64_t *allocations) {
    if (!sc) return fail(MCPT_ERR_ARG, "mcpt_scene_probe_buffers: null scene");
    const ProbeBufs &P = sc->probes;
    if (floats)
        *floats = (int64_t)(P.points.n + P.radiance.n +
                            4 * (P.relit_r0.n + P.relit_r1.n + P.relit_r2.n + P.relit_d.n + P.relit_ray_o.n + P.relit_ray_d.n + P.relit_slot.n + P.relit_hit.n));
    if (allocations) *allocations = sc->probes.allocations;
    return MCPT_OK;
}

int mcpt_sh_basis_host(int64_t n, const float *dirs, float *basis) {
    if (n < 0 || (n > 0 && (!dirs || !basis))) return fail(MCPT_ERR_ARG, "mcpt_sh_basis_host: n < 0, or null dirs or basis");
    for (int64_t i = 0; i < n; ++i) sh::sh9_basis(dirs + 3 * i, basis + 9 * i);
    return MCPT_OK;
}

int mcpt_sh_irradiance_host(int64_t n, const float *coef, const float *normals, float *out) {
    if (n < 0 || (n > 0 && (!coef || !normals || !out))) return fail(MCPT_ERR_ARG, "mcpt_sh_irradiance_host: n < 0, or null sh, normals or out");
    for (int64_t i = 0; i < n; ++i) sh::sh9_irradiance(coef + 27 * i, normals + 3 * i, out + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_grid_points_host(const mcpt_probe_grid *grid, float *points) {
    const std::string w = "mcpt_probe_grid_points_host";
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (!points) return fail(MCPT_ERR_ARG, w + ": null points");
    size_t i = 0;
    for (int32_t iz = 0; iz < g.dims[2]; ++iz)
        for (int32_t iy = 0; iy < g.dims[1]; ++iy)
            for (int32_t ix = 0; ix < g.dims[0]; ++ix, ++i) sh::grid_point(g, ix, iy, iz, points + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_shade_host(const mcpt_probe_grid *grid, const float *coef, int64_t n, const float *points, const float *normals, float *out) {
    const std::string w = "mcpt_probe_shade_host";
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (n < 0 || (n > 0 && (!coef || !points || !normals || !out))) return fail(MCPT_ERR_ARG, w + ": n < 0, or null sh, points, normals or out");
    for (int64_t i = 0; i < n; ++i) sh::probe_shade(g, coef, points + 3 * i, normals + 3 * i, out + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_depth_dirs_host(float *dirs) {
    if (!dirs) return fail(MCPT_ERR_ARG, "mcpt_probe_depth_dirs_host: null dirs");
    for (int32_t j = 0; j < pd::kTexels; ++j) pd::texel_dir(j, dirs + 3 * j);
    return MCPT_OK;
}

int mcpt_probe_depth_texel_host(int64_t n, const float *v, int32_t *texel) {
    if (n < 0 || (n > 0 && (!v || !texel))) return fail(MCPT_ERR_ARG, "mcpt_probe_depth_texel_host: n < 0, or null v or texel");
    for (int64_t i = 0; i < n; ++i) texel[i] = pd::texel_of(v + 3 * i);
    return MCPT_OK;
}

int mcpt_probe_depth_fold_host(int64_t n, int32_t spp, const float *dirs, const float *r, const uint8_t *backfacing, int32_t accumulate, float *moments,
                               int32_t *counts) {
    const std::string w = "mcpt_probe_depth_fold_host";
    if (n < 0 || n > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": n must be in 0 .. (2^31 - 1) / 192");
    if (spp <= 0) return fail(MCPT_ERR_ARG, w + ": spp must be positive");
    if (accumulate != 0 && accumulate != 1) return fail(MCPT_ERR_ARG, w + ": accumulate must be 0 or 1");
    if (n > 0 && (!dirs || !r || !backfacing || !moments || !counts)) return fail(MCPT_ERR_ARG, w + ": null dirs, r, backfacing, moments or counts");
    if (accumulate)
        for (int64_t i = 0; i < n; ++i)
            if (counts[2 * i] < 0 || (int64_t)counts[2 * i] + spp > 0x7fffffff) return fail(MCPT_ERR_ARG, w + ": spp does not fit the int32 counts together with the existing ones");
    float c[pd::kTexels][3];
    for (int32_t j = 0; j < pd::kTexels; ++j) pd::texel_dir(j, c[j]);
    for (int64_t i = 0; i < n; ++i) {
        const size_t s0 = (size_t)i * (size_t)spp;
        for (int32_t j = 0; j < pd::kTexels; ++j) {
            float *m3 = moments + ((size_t)i * pd::kTexels + j) * 3;
            float W = accumulate ? m3[0] : 0.f, S1 = accumulate ? m3[1] : 0.f, S2 = accumulate ? m3[2] : 0.f;
            for (int32_t k = 0; k < spp; ++k) pd::fold_sample(pd::fold_weight(c[j], dirs + 3 * (s0 + k)), r[s0 + k], W, S1, S2);
            m3[0] = W;
            m3[1] = S1;
            m3[2] = S2;
        }
        int32_t back = 0;
        for (int32_t k = 0; k < spp; ++k) back += backfacing[s0 + k] ? 1 : 0;
        counts[2 * i] = (accumulate ? counts[2 * i] : 0) + spp;
        counts[2 * i + 1] = (accumulate ? counts[2 * i + 1] : 0) + back;
    }
    return MCPT_OK;
}

int mcpt_rng_uniforms_host(uint32_t seed, uint32_t pixel, int64_t n, const uint32_t *sample, const uint32_t *depth, const uint32_t *block,
                           const uint32_t *stream, float *out) {
    if (n < 0 || (n > 0 && (!sample || !depth || !block || !stream || !out)))
        return fail(MCPT_ERR_ARG, "mcpt_rng_uniforms_host: n < 0, or null sample, depth, block, stream or out");
    for (int64_t i = 0; i < n; ++i) rng_block(RngKey{seed, pixel, sample[i], stream[i]}, depth[i], block[i], out + 4 * i);
    return MCPT_OK;
}

int mcpt_direct_samples_host(int64_t n, int32_t N, const float *points, const float *normals, const float *light_rows, float *q_out, float *ws_out,
                             float *dist_out, uint8_t *live_out, float *contrib_out) {
    const std::string w = "mcpt_direct_samples_host";
    if (N < 1 || N > dl::kMaxSamples) return fail(MCPT_ERR_ARG, w + ": N must be in 1 .. 4096");
    if (n < 0 || n > (int64_t)0x7fffffff / N) return fail(MCPT_ERR_ARG, w + ": n must not be negative and n * N at most 2^31 - 1");
    if (n > 0 && (!points || !normals || !light_rows || !q_out || !ws_out || !dist_out || !live_out || !contrib_out))
        return fail(MCPT_ERR_ARG, w + ": null points, normals, light_rows or output");
    dl::samples_host(n, N, points, normals, light_rows, q_out, ws_out, dist_out, live_out, contrib_out);
    return MCPT_OK;
}

int mcpt_direct_fold_host(int64_t n, int32_t N, const float *contrib, const uint8_t *visible, float *out) {
    const std::string w = "mcpt_direct_fold_host";
    if (N < 1 || N > dl::kMaxSamples) return fail(MCPT_ERR_ARG, w + ": N must be in 1 .. 4096");
    if (n < 0 || n > (int64_t)0x7fffffff / N) return fail(MCPT_ERR_ARG, w + ": n must not be negative and n * N at most 2^31 - 1");
    if (n > 0 && (!contrib || !visible || !out)) return fail(MCPT_ERR_ARG, w + ": null contrib, visible or out");
    dl::fold_host(n, N, contrib, visible, out);
    return MCPT_OK;
}

int mcpt_probe_shade_visible_host(const mcpt_probe_grid *grid, const float *coef, const float *moments, const int32_t *counts,
                                  const mcpt_probe_visibility *opts, int64_t n, const float *points, const float *normals, float *out, float *weight_out) {
    const std::string w = "mcpt_probe_shade_visible_host";
    sh::Grid g;
    const int c = check_grid(w, grid, g);
    if (c != MCPT_OK) return c;
    if (grid_probes(g) > (int64_t)pd::kMaxProbes) return fail(MCPT_ERR_ARG, w + ": dims must name at most (2^31 - 1) / 192 probes");
    const int vc = check_visibility(w, opts);
    if (vc != MCPT_OK) return vc;
    if (n < 0 || (n > 0 && (!coef || !moments || !counts || !points || !normals || !out)))
        return fail(MCPT_ERR_ARG, w + ": n < 0, or null sh, moments, counts, points, normals or out");
    for (int64_t i = 0; i < n; ++i)
        pd::shade_visible(g, coef, moments, counts, opts->normal_bias, opts->backface_max, points + 3 * i, normals + 3 * i, out + 3 * i,
                          weight_out ? weight_out + i : nullptr);
    return MCPT_OK;
}

}  // extern "C"
