// Sky-pixel culling (csrc/mcpt_cull.hip): conservative per-pixel classification before the wavefront loop.
#pragma once
#include <hip/hip_runtime.h>

#include "mcpt_kernels.h"

namespace mcpt {

// The host half of the classification (the header comment of mcpt_cull.hip derives it): what k_classify gets besides the camera.
struct CullBound {
    bool classified;                  // false: the camera is outside what the bound covers; nothing is culled and rho is not used
    float rho;                        // widening of every box, as the kernel gets it
    float scale, aspect, focal, lens; // CullConst: focal distance (1 without DoF), aperture radius (0 without DoF)
    double h, s_far, reach, fmin;     // 0 where the refusal came before they were formed
};
CullBound cull_bound(const CameraConst &cam, const float root_min[3], const float root_max[3]);
inline void fill_cull_info(const CullBound &b, mcpt_cull_info *info) {
    info->classified = b.classified ? 1 : 0;
    info->rho = b.rho;
    info->scale = b.scale;
    info->aspect = b.aspect;
    info->focal = b.focal;
    info->lens = b.lens;
    info->h = b.h;
    info->s_far = b.s_far;
    info->reach = b.reach;
    info->fmin = b.fmin;
}

// Partitions the n owned pixels `d_pixels` into d_out[0, *n_trace) (pixels whose rays may hit something, original order) and
// d_out[*n_trace, n) (pixels that can only see the background).  d_flags: n bytes, d_temp / temp_bytes: cull_temp_bytes(n),
// d_count: one uint32.  Leaves *n_trace == n (nothing culled, d_out untouched) for cameras the bound does not cover.  Synchronises `st`.
// d_cand_out (aligned with d_out): per pixel the at most four primitives its rays can hit (leaf references, kCandNone = unused), or
// kCandTraverse in .x; d_cand_tmp: n entries of scratch.  d_flags and d_cand_tmp keep what k_classify wrote, in the order of d_pixels.
// rho_scale multiplies the final rho in the checking build only (Knobs::cull_rho_scale); used (nullable) receives the bound as applied.
hipError_t cull_sky_pixels(const DevScene &S, const CameraConst &cam, const uint32_t *d_pixels, uint32_t n, uint32_t *d_out, uint8_t *d_flags,
                           int4 *d_cand_tmp, int4 *d_cand_out, void *d_temp, size_t temp_bytes, uint32_t *d_count, uint32_t *n_trace, float rho_scale,
                           CullBound *used, hipStream_t st);
size_t cull_temp_bytes(uint32_t n);
// framebuffer[m][c] += background[c] / spp_total, spp times in order, for the culled pixels (what the wavefront would accumulate)
void launch_sky_fill(const uint32_t *sky_pixels, uint32_t n_sky, const float background[3], int32_t spp, float spp_total, float *fb, hipStream_t st);

}  // namespace mcpt
