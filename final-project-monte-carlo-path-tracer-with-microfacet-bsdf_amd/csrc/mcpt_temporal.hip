// Temporal reuse (include/mcpt.h: mcpt_render_motion, mcpt_temporal_blend); csrc/mcpt_temporal.h has the arithmetic, shared with the
// CPU build the tests compare against.
//
// Motion pass: the AOV pass's chunk loop (csrc/mcpt_render.hip: keys, camera rays, closest hits) with two kernels of its own
//   k_motion_resolve  hit -> per-sample record {dx, dy, prev_depth, valid}: the hit point rebuilt on the live primitive and on the
//                     snapshot's, both projected
//   k_motion_fold     one lane per pixel: the samples folded in sample order into the 4-float motion record
// With specular_depth > 0 (mcpt_render_motion_ex) k_motion_chain takes k_motion_resolve's place, as k_aov_chain takes k_aov_resolve's
// (csrc/mcpt_denoise.hip): the same lists, the same bounce (csrc/mcpt_chain.h), the same compaction; a sample that reflects composes the
// mirror plane into its two maps (csrc/mcpt_specular_motion.h), one that stops writes its record from the unfolded terminal hit.
// The pixel rule (tp::reuse_pixel, once, with compile-time switches) over a frame: 16 x 16 pixel blocks, one pixel per lane; a wave covers
// four rows of 16 pixels, so its loads of the pixel's own colour, motion and its stores are four contiguous runs; up to four taps of the
// previous frame per lane, no LDS (neighbouring lanes' taps are neighbouring pixels: the cache lines are shared in L1 / L2).  Three kernels
// of that shape, every store a plain vector store:
//   k_temporal_blend  the blend (mcpt_temporal_blend)
//   k_temporal_accumulate<kNorm, kClamp>  the blend with the variance of its result (mcpt_temporal_accumulate[_ex], mcpt_sequence_frame):
//                     four instantiations over the two switches of history rejection, picked by the launcher, so no lane branches on a
//                     switch.  <false, false> is the plain accumulation; kNorm adds the normal test on every tap, kClamp the clamp of the
//                     history to the 3 x 3 neighbourhood of the new frame.  The nine neighbours are read straight from global memory: a
//                     lane's row neighbours are its wave neighbours' own pixels, so the 36-byte runs overlap in L1 (a 16 x 16 tile touches
//                     18 x 18 pixels, 1.27 x its own colour bytes); an LDS tile with a halo would add a barrier and a second pass over the
//                     halo to save loads that already hit.  Every instantiation copies the frame's first-hit depth into the next history
//                     set, and kNorm the first-hit normal where that set has a normal plane, so that one launch leaves the history
//                     complete for the next frame; with a switch on it writes the flags byte where there is a flags plane.
//                     k_temporal_accumulate<kNorm, kClamp, true> are the four kWeight instantiations (mcpt_temporal_accumulate_weighted, a
//                     sequence created with weighted 1): one more load per tap (the history weight), the pixel's count or the uniform
//                     one, and one more store, the new weight; 8 bytes per pixel of traffic.  The weight-off instantiations are the four
//                     there have always been.  k_temporal_accumulate<kNorm, kClamp, false, true> are the four kMoments instantiations
//                     (mcpt_temporal_accumulate_moments, a sequence created with moments): no variance plane read or written; one
//                     8-byte load per tap (the history's luminance moments) and one 8-byte store, 16 bytes per pixel of traffic in
//                     place of the 12 of the three variance accesses.
//   k_history_len     the guide of an adaptive sequence (mcpt_temporal_history_len, mcpt_sequence_create_adaptive with guided 1):
//                     tp::history_len_pixel, the taps and skips of the rule without its colour, known before the frame is rendered.
//   k_history_weight  the same for a weighted sequence (mcpt_temporal_history_weight): tp::history_weight_pixel, the smallest history
//                     weight of the taps the kWeight flavour will use.
#include <hip/hip_runtime.h>

#include "mcpt_chain.h"
#include "mcpt_temporal.h"

namespace mcpt {

namespace {

constexpr int kB = 256;
constexpr int kTile = 16;
inline uint32_t nblocks(uint32_t n) { return (n + kB - 1) / kB; }
// tp::tri_point reads a TriGeom as nine floats v0, e1, e2
static_assert(offsetof(TriGeom, e1x) == 12 && offsetof(TriGeom, e1yz) == 16 && offsetof(TriGeom, e2xy) == 24 && offsetof(TriGeom, e2z) == 32, "TriGeom layout");

// Where the hit of ray (ro, rd) on primitive prim is now (pc) and was in the snapshot (pp): the first-hit rule of mcpt_render_motion.
// Triangles: the barycentrics of the test that recorded the hit (it succeeds again; false if not), each rounded once to float, on the live
// record g and on the snapshot's.  Spheres: o + d (float)t, moved with the centre.
MCPT_DI bool hit_points(const DevScene &S, const TriGeom *__restrict__ prev_tri, const SphereRec *__restrict__ prev_sph, int32_t prim, const uint4 &h,
                        f3 ro, f3 rd, float pc[3], float pp[3]) {
    if (prim < S.n_tri) {
        const TriGeom g = S.tri_geom[prim];
        double tt, u, v;
        if (!tri_hit(g, make_ray(ro, rd), tt, u, v)) return false;
        tp::tri_point(reinterpret_cast<const float *>(&g), (float)u, (float)v, pc);
        tp::tri_point(reinterpret_cast<const float *>(prev_tri + prim), (float)u, (float)v, pp);
    } else {
        const f3 p = ro + rd * (float)hit_t(h);
        const SphereRec &sc = S.spheres[prim - S.n_tri], &sp = prev_sph[prim - S.n_tri];
        pc[0] = p.x;
        pc[1] = p.y;
        pc[2] = p.z;
        pp[0] = p.x + (sp.c[0] - sc.c[0]);
        pp[1] = p.y + (sp.c[1] - sc.c[1]);
        pp[2] = p.z + (sp.c[2] - sc.c[2]);
    }
    return true;
}

__global__ __launch_bounds__(kB) void k_motion_resolve(DevScene S, const TriGeom *__restrict__ prev_tri, const SphereRec *__restrict__ prev_sph,
                                                       tp::Cam cur, tp::Cam prev, uint32_t n, const float4 *__restrict__ ray_o,
                                                       const float4 *__restrict__ ray_d, const uint4 *__restrict__ hit, float4 *__restrict__ rec) {
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    if (j >= n) return;
    const uint4 h = hit[j];
    const int32_t prim = (int32_t)h.z;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    if (prim >= 0) {
        const float4 o4 = ray_o[j], d4 = ray_d[j];
        float pc[3], pp[3];
        if (hit_points(S, prev_tri, prev_sph, prim, h, mk3(o4.x, o4.y, o4.z), mk3(d4.x, d4.y, d4.z), pc, pp)) tp::sample_motion(cur, prev, pc, pp, out);
    }
    rec[j] = make_float4(out[0], out[1], out[2], out[3]);
}

// The two maps of sample j: six float4, plane k of `stride` entries at maps + k stride (A_cur rows 0-2, then A_prev rows 0-2).
MCPT_DI void load_maps(const float4 *__restrict__ maps, size_t stride, uint32_t j, float Ac[12], float Ap[12]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 a = maps[k * stride + j], b = maps[(3 + k) * stride + j];
        Ac[4 * k] = a.x, Ac[4 * k + 1] = a.y, Ac[4 * k + 2] = a.z, Ac[4 * k + 3] = a.w;
        Ap[4 * k] = b.x, Ap[4 * k + 1] = b.y, Ap[4 * k + 2] = b.z, Ap[4 * k + 3] = b.w;
    }
}
MCPT_DI void store_maps(float4 *__restrict__ maps, size_t stride, uint32_t j, const float Ac[12], const float Ap[12]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        maps[k * stride + j] = make_float4(Ac[4 * k], Ac[4 * k + 1], Ac[4 * k + 2], Ac[4 * k + 3]);
        maps[(3 + k) * stride + j] = make_float4(Ap[4 * k], Ap[4 * k + 1], Ap[4 * k + 2], Ap[4 * k + 3]);
    }
}

// One step of the specular chains of the motion pass (include/mcpt.h: mcpt_render_motion_ex) for the n rays of a list whose samples have all
// followed b bounces; the shape of k_aov_chain (csrc/mcpt_denoise.hip).  Ray i belongs to sample j, which has composed n_refl reflections into
// its maps (chain_in[i] = {n_refl bits, -, -, j bits}; nullptr for the camera rays: j = i, n_refl = 0).  A sample that stops writes its record
// rec[j] from its terminal hit, unfolded through its maps; one that follows a Dirac bounce (b < max_b) appends its next ray and state to the
// next list (ballot + prefix count, one atomic per wave on n_next) and, if it reflects, composes the mirror plane into maps[.. j]: only
// sample j's lane ever touches entry j, so one array serves every bounce.
__global__ __launch_bounds__(kB) void k_motion_chain(DevScene S, const TriGeom *__restrict__ prev_tri, const SphereRec *__restrict__ prev_sph,
                                                     tp::Cam cur, tp::Cam prev, uint32_t n, int32_t b, int32_t max_b,
                                                     const float4 *__restrict__ ray_o, const float4 *__restrict__ ray_d, const uint4 *__restrict__ hit,
                                                     const float4 *__restrict__ chain_in, float4 *__restrict__ rec, float4 *__restrict__ maps,
                                                     size_t map_stride, float4 *__restrict__ next_o, float4 *__restrict__ next_d,
                                                     float4 *__restrict__ chain_out, uint32_t *__restrict__ n_next) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    bool cont = false;  // (no early return: every lane takes part in the ballot)
    uint32_t j = i;
    int32_t n_refl = 0;
    f3 p2 = mk3(0, 0, 0), wi = mk3(0, 0, 1);
    if (i < n) {
        if (chain_in) {
            const float4 c = chain_in[i];
            n_refl = (int32_t)__float_as_uint(c.x);
            j = __float_as_uint(c.w);
        }
        const uint4 h = hit[i];
        const int32_t prim = (int32_t)h.z;
        float out[4] = {0.f, 0.f, 0.f, 0.f};
        if (prim >= 0) {
            const float4 o4 = ray_o[i], d4 = ray_d[i];
            const f3 ro = mk3(o4.x, o4.y, o4.z), rd = mk3(d4.x, d4.y, d4.z);
            const f3 p = ro + rd * (float)hit_t(h);
            f3 nrm;
            if (prim < S.n_tri) {
                const float *tn = S.tri_shade[prim].n;
                nrm = mk3(tn[0], tn[1], tn[2]);
            } else {
                const float *c = S.spheres[prim - S.n_tri].c;
                nrm = normalized(p - mk3(c[0], c[1], c[2]));
            }
            const MaterialRec &M = S.mats[h.w & kMatIndexMask];
            cont = chain_continues(M, h.w, b, max_b);
            float Ac[12], Ap[12];
            if (cont) {
                if (chain_bounce(M, rd, p, nrm, p2, wi)) {
                    if (n_refl > 0) load_maps(maps, map_stride, j, Ac, Ap);
                    if (prim < S.n_tri) {
                        const TriGeom g = S.tri_geom[prim];
                        double tt, u, v;
                        if (tri_hit(g, make_ray(ro, rd), tt, u, v))  // (the test that recorded the hit: it succeeds again)
                            tp::chain_reflect_tri(Ac, Ap, n_refl, reinterpret_cast<const float *>(&g), reinterpret_cast<const float *>(prev_tri + prim),
                                                  (float)u, (float)v);
                        else
                            cont = false;  // (as k_motion_resolve: no record without the barycentrics)
                    } else {
                        const float pf[3] = {p.x, p.y, p.z}, nf[3] = {nrm.x, nrm.y, nrm.z};
                        tp::chain_reflect_sphere(Ac, Ap, n_refl, pf, nf, S.spheres[prim - S.n_tri].c, prev_sph[prim - S.n_tri].c);
                    }
                    if (cont) store_maps(maps, map_stride, j, Ac, Ap);
                    ++n_refl;
                }
            } else {
                float qc[3], qp[3];
                if (hit_points(S, prev_tri, prev_sph, prim, h, ro, rd, qc, qp)) {
                    if (n_refl > 0) load_maps(maps, map_stride, j, Ac, Ap);
                    tp::chain_motion(cur, prev, Ac, Ap, n_refl, qc, qp, out);
                }
            }
        }
        if (!cont) rec[j] = make_float4(out[0], out[1], out[2], out[3]);
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
        chain_out[k] = make_float4(__uint_as_float((uint32_t)n_refl), 0.f, 0.f, __uint_as_float(j));
    }
}

__global__ __launch_bounds__(kB) void k_motion_fold(uint32_t p0, uint32_t n_pix, int32_t spp, const float4 *__restrict__ rec, float *__restrict__ motion) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_pix) return;
    float out[4];
    tp::fold_pixel(reinterpret_cast<const float *>(rec + (size_t)i * spp), spp, out);
    reinterpret_cast<float4 *>(motion)[p0 + i] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(kTile *kTile) void k_temporal_blend(int W, int H, tp::Opts o, tp::Frame f, tp::Prev p, tp::Next n) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    tp::blend_pixel(W, H, x, y, f, p, o, n);
}

template <bool kNorm, bool kClamp, bool kWeight, bool kMoments>
__global__ __launch_bounds__(kTile *kTile) void k_temporal_accumulate(int W, int H, tp::Opts o, tp::HistOpts ho, tp::Frame f, tp::Prev p, tp::Next n, tp::Moments mo) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t m = (size_t)y * W + x;
    tp::store_pixel<!kMoments, kNorm || kClamp, kWeight, kMoments>(n, m, tp::reuse_pixel<!kMoments, kNorm, kClamp, kWeight, kMoments>(W, H, x, y, f, p, o, ho, mo), mo.next);
    if (f.depth) n.depth[m] = f.depth[m * (size_t)f.depth_stride];
    if (kNorm && n.normal) {  // (nothing reads the normals without the normal test; three loads, then three stores: one round trip)
        const float *fn = f.normal + m * (size_t)f.normal_stride;
        const float n0 = fn[0], n1 = fn[1], n2 = fn[2];
        n.normal[m * 3] = n0, n.normal[m * 3 + 1] = n1, n.normal[m * 3 + 2] = n2;
    }
}

__global__ __launch_bounds__(kTile *kTile) void k_history_len(int W, int H, tp::Opts o, tp::HistOpts ho, tp::Frame f, tp::Prev p, float *__restrict__ len) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    len[(size_t)y * W + x] = tp::history_len_pixel(W, H, x, y, f, p, o, ho);
}

__global__ __launch_bounds__(kTile *kTile) void k_history_weight(int W, int H, tp::Opts o, tp::HistOpts ho, tp::Frame f, tp::Prev p, float *__restrict__ weight) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    weight[(size_t)y * W + x] = tp::history_weight_pixel(W, H, x, y, f, p, o, ho);
}

template <bool kWeight, bool kMoments>
auto accumulate_kernel(const tp::HistOpts &ho) {
    return ho.normal_test ? (ho.color_clamp ? k_temporal_accumulate<true, true, kWeight, kMoments> : k_temporal_accumulate<true, false, kWeight, kMoments>)
                          : (ho.color_clamp ? k_temporal_accumulate<false, true, kWeight, kMoments> : k_temporal_accumulate<false, false, kWeight, kMoments>);
}

inline dim3 tiles(int W, int H) { return dim3((W + kTile - 1) / kTile, (H + kTile - 1) / kTile); }

}  // namespace

void launch_motion_resolve(const DevScene &S, const TriGeom *prev_tri, const SphereRec *prev_sph, const tp::Cam &cur, const tp::Cam &prev, uint32_t n,
                           const float4 *ray_o, const float4 *ray_d, const uint4 *hit, float4 *rec, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_motion_resolve, dim3(nblocks(n)), dim3(kB), 0, st, S, prev_tri, prev_sph, cur, prev, n, ray_o, ray_d, hit, rec);
}

void launch_motion_chain(const DevScene &S, const TriGeom *prev_tri, const SphereRec *prev_sph, const tp::Cam &cur, const tp::Cam &prev, uint32_t n, int32_t b,
                         int32_t max_b, const float4 *ray_o, const float4 *ray_d, const uint4 *hit, const float4 *chain_in, float4 *rec, float4 *maps,
                         size_t map_stride, float4 *next_o, float4 *next_d, float4 *chain_out, uint32_t *n_next, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_motion_chain, dim3(nblocks(n)), dim3(kB), 0, st, S, prev_tri, prev_sph, cur, prev, n, b, max_b, ray_o, ray_d, hit, chain_in, rec,
                       maps, map_stride, next_o, next_d, chain_out, n_next);
}

void launch_motion_fold(uint32_t p0, uint32_t n_pix, int32_t spp, const float4 *rec, float *motion, hipStream_t st) {
    if (n_pix == 0) return;
    hipLaunchKernelGGL(k_motion_fold, dim3(nblocks(n_pix)), dim3(kB), 0, st, p0, n_pix, spp, rec, motion);
}

void launch_temporal_blend(int W, int H, const tp::Opts &o, const tp::Frame &f, const tp::Prev &p, const tp::Next &n, hipStream_t st) {
    hipLaunchKernelGGL(k_temporal_blend, tiles(W, H), dim3(kTile, kTile), 0, st, W, H, o, f, p, n);
}

void launch_temporal_accumulate(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, const tp::Next &n,
                                hipStream_t st) {
    const auto k = n.weight ? accumulate_kernel<true, false>(ho) : accumulate_kernel<false, false>(ho);
    hipLaunchKernelGGL(k, tiles(W, H), dim3(kTile, kTile), 0, st, W, H, o, ho, f, p, n, tp::Moments{});
}

void launch_temporal_accumulate_moments(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, const tp::Next &n,
                                        const tp::Moments &mo, hipStream_t st) {
    hipLaunchKernelGGL((accumulate_kernel<false, true>(ho)), tiles(W, H), dim3(kTile, kTile), 0, st, W, H, o, ho, f, p, n, mo);
}

void launch_history_len(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, float *len, hipStream_t st) {
    hipLaunchKernelGGL(k_history_len, tiles(W, H), dim3(kTile, kTile), 0, st, W, H, o, ho, f, p, len);
}

void launch_history_weight(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const tp::Frame &f, const tp::Prev &p, float *weight, hipStream_t st) {
    hipLaunchKernelGGL(k_history_weight, tiles(W, H), dim3(kTile, kTile), 0, st, W, H, o, ho, f, p, weight);
}

}  // namespace mcpt
