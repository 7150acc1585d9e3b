// Temporal reuse (include/mcpt.h: mcpt_render_motion, mcpt_temporal_blend); csrc/mcpt_temporal.h has the arithmetic, shared with the
// CPU build the tests compare against.
//
// Motion pass: the AOV pass's chunk loop (csrc/mcpt_render.hip: keys, camera rays, closest hits) with two kernels of its own
//   k_motion_resolve  hit -> per-sample record {dx, dy, prev_depth, valid}: the hit point rebuilt on the live primitive and on the
//                     snapshot's, both projected
//   k_motion_fold     one lane per pixel: the samples folded in sample order into the 4-float motion record
// Blend:
//   k_temporal_blend  16 x 16 pixel blocks, one pixel per lane; a wave covers four rows of 16 pixels, so its loads of the pixel's own
//                     colour, motion and its stores are four contiguous runs; up to four taps of the previous frame per lane, no LDS
//                     (neighbouring lanes' taps are neighbouring pixels: the cache lines are shared in L1 / L2)
// Accumulate (mcpt_temporal_accumulate, mcpt_sequence_frame):
//   k_temporal_accumulate  the same shape; the blend with the variance of its result (tp::accumulate_pixel), and the frame's first-hit
//                     depth copied into the history's depth plane, so that one launch leaves the history complete for the next frame
// Accumulate with history rejection (mcpt_temporal_accumulate_ex, a sequence created with mcpt_sequence_create_ex):
//   k_temporal_accumulate_ex  the same shape again; tp::accumulate_pixel_ex adds the normal test on every tap and the clamp of the history
//                     to the 3 x 3 neighbourhood of the new frame.  The nine neighbours are read straight from global memory: a lane's row
//                     neighbours are its wave neighbours' own pixels, so the 36-byte runs overlap in L1 (a 16 x 16 tile touches 18 x 18
//                     pixels, 1.27 x its own colour bytes); an LDS tile with a halo would add a barrier and a second pass over the halo
//                     to save loads that already hit.  It also copies the frame's first-hit normal into the history's normal plane and
//                     writes the flags byte, both with plain vector stores.
// Guide of an adaptive sequence (mcpt_temporal_history_len, a sequence created with mcpt_sequence_create_adaptive, guided 1):
//   k_history_len     the same shape; tp::history_len_pixel: the taps and skips of the blend without its colour, so the length a pixel is
//                     about to get is known before the frame is rendered.  One plain vector store per lane.
#include <hip/hip_runtime.h>

#include "mcpt_temporal.h"

namespace mcpt {

namespace {

constexpr int kB = 256;
constexpr int kTile = 16;
inline uint32_t nblocks(uint32_t n) { return (n + kB - 1) / kB; }
// tp::tri_point reads a TriGeom as nine floats v0, e1, e2
static_assert(offsetof(TriGeom, e1x) == 12 && offsetof(TriGeom, e1yz) == 16 && offsetof(TriGeom, e2xy) == 24 && offsetof(TriGeom, e2z) == 32, "TriGeom layout");

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
        const f3 ro = mk3(o4.x, o4.y, o4.z), rd = mk3(d4.x, d4.y, d4.z);
        float pc[3], pp[3];
        bool ok = true;
        if (prim < S.n_tri) {
            const TriGeom g = S.tri_geom[prim];
            double tt, u, v;
            ok = tri_hit(g, make_ray(ro, rd), tt, u, v);  // (the test that recorded the hit: it succeeds again)
            if (ok) {
                tp::tri_point(reinterpret_cast<const float *>(&g), (float)u, (float)v, pc);
                tp::tri_point(reinterpret_cast<const float *>(prev_tri + prim), (float)u, (float)v, pp);
            }
        } else {
            const double t = __longlong_as_double((long long)(((unsigned long long)h.y << 32) | h.x));
            const f3 p = ro + rd * (float)t;
            const SphereRec &sc = S.spheres[prim - S.n_tri], &sp = prev_sph[prim - S.n_tri];
            pc[0] = p.x;
            pc[1] = p.y;
            pc[2] = p.z;
            pp[0] = p.x + (sp.c[0] - sc.c[0]);
            pp[1] = p.y + (sp.c[1] - sc.c[1]);
            pp[2] = p.z + (sp.c[2] - sc.c[2]);
        }
        if (ok) tp::sample_motion(cur, prev, pc, pp, out);
    }
    rec[j] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(kB) void k_motion_fold(uint32_t p0, uint32_t n_pix, int32_t spp, const float4 *__restrict__ rec, float *__restrict__ motion) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_pix) return;
    float out[4];
    tp::fold_pixel(reinterpret_cast<const float *>(rec + (size_t)i * spp), spp, out);
    reinterpret_cast<float4 *>(motion)[p0 + i] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(kTile *kTile) void k_temporal_blend(int W, int H, tp::Opts o, const float *__restrict__ color, const float *__restrict__ motion,
                                                                const float *__restrict__ prev_color, const float *__restrict__ prev_depth,
                                                                const float *__restrict__ prev_len, float *__restrict__ out_color,
                                                                float *__restrict__ out_len) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    tp::blend_pixel(W, H, x, y, color, motion, prev_color, prev_depth, prev_len, o, out_color, out_len);
}

__global__ __launch_bounds__(kTile *kTile) void k_temporal_accumulate(int W, int H, tp::Opts o, const float *__restrict__ color, const float *__restrict__ variance,
                                                                     const float *__restrict__ motion, const float *__restrict__ prev_color,
                                                                     const float *__restrict__ prev_variance, const float *__restrict__ prev_depth,
                                                                     const float *__restrict__ prev_len, const float *__restrict__ depth, int depth_stride,
                                                                     float *__restrict__ out_color, float *__restrict__ out_variance,
                                                                     float *__restrict__ out_depth, float *__restrict__ out_len) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    tp::accumulate_pixel(W, H, x, y, color, variance, motion, prev_color, prev_variance, prev_depth, prev_len, o, out_color, out_variance, out_len);
    const size_t m = (size_t)y * W + x;
    if (depth) out_depth[m] = depth[m * (size_t)depth_stride];
}

__global__ __launch_bounds__(kTile *kTile) void k_temporal_accumulate_ex(
    int W, int H, tp::Opts o, tp::HistOpts ho, const float *__restrict__ color, const float *__restrict__ variance, const float *__restrict__ motion,
    const float *__restrict__ normal, int normal_stride, const float *__restrict__ prev_color, const float *__restrict__ prev_variance,
    const float *__restrict__ prev_depth, const float *__restrict__ prev_len, const float *__restrict__ prev_normal, const float *__restrict__ depth,
    int depth_stride, float *__restrict__ out_color, float *__restrict__ out_variance, float *__restrict__ out_depth, float *__restrict__ out_len,
    float *__restrict__ out_normal, uint8_t *__restrict__ out_flags) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    tp::accumulate_pixel_ex(W, H, x, y, color, variance, motion, normal, normal_stride, prev_color, prev_variance, prev_depth, prev_len, prev_normal, o, ho,
                            out_color, out_variance, out_len, out_flags);
    const size_t m = (size_t)y * W + x;
    if (depth) out_depth[m] = depth[m * (size_t)depth_stride];
    if (out_normal) {
        const float *n = normal + m * (size_t)normal_stride;
        out_normal[m * 3] = n[0];
        out_normal[m * 3 + 1] = n[1];
        out_normal[m * 3 + 2] = n[2];
    }
}

__global__ __launch_bounds__(kTile *kTile) void k_history_len(int W, int H, tp::Opts o, tp::HistOpts ho, const float *__restrict__ motion,
                                                              const float *__restrict__ normal, int normal_stride, const float *__restrict__ prev_color,
                                                              const float *__restrict__ prev_depth, const float *__restrict__ prev_len,
                                                              const float *__restrict__ prev_normal, float *__restrict__ len) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    len[(size_t)y * W + x] = tp::history_len_pixel(W, H, x, y, motion, normal, normal_stride, prev_color, prev_depth, prev_len, prev_normal, o, ho);
}

}  // namespace

void launch_motion_resolve(const DevScene &S, const TriGeom *prev_tri, const SphereRec *prev_sph, const tp::Cam &cur, const tp::Cam &prev, uint32_t n,
                           const float4 *ray_o, const float4 *ray_d, const uint4 *hit, float4 *rec, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_motion_resolve, dim3(nblocks(n)), dim3(kB), 0, st, S, prev_tri, prev_sph, cur, prev, n, ray_o, ray_d, hit, rec);
}

void launch_motion_fold(uint32_t p0, uint32_t n_pix, int32_t spp, const float4 *rec, float *motion, hipStream_t st) {
    if (n_pix == 0) return;
    hipLaunchKernelGGL(k_motion_fold, dim3(nblocks(n_pix)), dim3(kB), 0, st, p0, n_pix, spp, rec, motion);
}

void launch_temporal_blend(int W, int H, const tp::Opts &o, const float *color, const float *motion, const float *prev_color, const float *prev_depth,
                           const float *prev_len, float *out_color, float *out_len, hipStream_t st) {
    const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), blk(kTile, kTile);
    hipLaunchKernelGGL(k_temporal_blend, grid, blk, 0, st, W, H, o, color, motion, prev_color, prev_depth, prev_len, out_color, out_len);
}

void launch_temporal_accumulate(int W, int H, const tp::Opts &o, const float *color, const float *variance, const float *motion, const float *prev_color,
                                const float *prev_variance, const float *prev_depth, const float *prev_len, const float *depth, int depth_stride,
                                float *out_color, float *out_variance, float *out_depth, float *out_len, hipStream_t st) {
    const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), blk(kTile, kTile);
    hipLaunchKernelGGL(k_temporal_accumulate, grid, blk, 0, st, W, H, o, color, variance, motion, prev_color, prev_variance, prev_depth, prev_len, depth,
                       depth_stride, out_color, out_variance, out_depth, out_len);
}

void launch_temporal_accumulate_ex(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const float *color, const float *variance, const float *motion,
                                   const float *normal, int normal_stride, const float *prev_color, const float *prev_variance, const float *prev_depth,
                                   const float *prev_len, const float *prev_normal, const float *depth, int depth_stride, float *out_color,
                                   float *out_variance, float *out_depth, float *out_len, float *out_normal, uint8_t *out_flags, hipStream_t st) {
    const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), blk(kTile, kTile);
    hipLaunchKernelGGL(k_temporal_accumulate_ex, grid, blk, 0, st, W, H, o, ho, color, variance, motion, normal, normal_stride, prev_color, prev_variance,
                       prev_depth, prev_len, prev_normal, depth, depth_stride, out_color, out_variance, out_depth, out_len, out_normal, out_flags);
}

void launch_history_len(int W, int H, const tp::Opts &o, const tp::HistOpts &ho, const float *motion, const float *normal, int normal_stride,
                        const float *prev_color, const float *prev_depth, const float *prev_len, const float *prev_normal, float *len, hipStream_t st) {
    const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), blk(kTile, kTile);
    hipLaunchKernelGGL(k_history_len, grid, blk, 0, st, W, H, o, ho, motion, normal, normal_stride, prev_color, prev_depth, prev_len, prev_normal, len);
}

}  // namespace mcpt
