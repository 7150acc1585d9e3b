// Adaptive sampling (csrc/mcpt_adaptive.hip): the per-round selection of mcpt_render_adaptive.
#pragma once
#include <hip/hip_runtime.h>

#include "mcpt_kernels.h"

namespace mcpt {

// Moments of the pixels the sky cull finished (every sample equals background[c]): moments[6m + c] and moments[6m + 3 + c] = the sums of
// v and v*v over spp samples, in double and in sample order, as k_accumulate<true> would have added them.
void launch_sky_moments(const uint32_t *sky_pixels, uint32_t n_sky, const float background[3], int32_t spp, double *moments, hipStream_t st);
// Pass 1, one lane per listed pixel with n samples: e = the stopping rule's estimate (include/mcpt.h), err[m] = (float)e, spp_map[m] = n;
// stamp != nullptr: stamp[m] = (round_stamp << 1) | (e > threshold), the mark its neighbours read in pass 2.  guide != nullptr (W*H floats):
// the pixel's threshold is threshold * sqrt(g) in double, g = guide[m] >= 1 ? guide[m] : 1 (tp::guided_threshold); err stays the unscaled e.
// weight_max_history > 0 (with a guide): the plane holds history weights H and the threshold is threshold * sqrt((double)
// tp::weight_guide(H[m], n, weight_max_history)) (mcpt_render_adaptive_weighted); 0: the plane holds history lengths.
void launch_adapt_eval(const uint32_t *list, uint32_t n_list, const double *moments, int32_t n, double rel_floor, double threshold, const float *guide,
                       float weight_max_history, uint32_t round_stamp, float *err, uint8_t *stamp, int32_t *spp_map, hipStream_t st);
// Pass 2: a listed pixel continues iff can_double and (its own mark, or with dilate a mark of an 8-neighbour stamped this round).
// A continuing pixel's fb is scaled by 0.5 and spp_map[m] = 2n; flags[i] = 1 for continuing list entries, 0 otherwise.
void launch_adapt_select(const uint32_t *list, uint32_t n_list, int width, int height, const uint8_t *stamp, uint32_t round_stamp, int dilate,
                         int can_double, int32_t n, float *fb, int32_t *spp_map, uint8_t *flags, hipStream_t st);
// Keeps the flagged entries of list (and of cand, when not null) in order: out[0, *n_out), cand_out likewise.  d_temp: adapt_temp_bytes(n).
// Synchronises `st` to read the count back.
hipError_t adapt_compact(const uint32_t *list, const int4 *cand, const uint8_t *flags, uint32_t n, uint32_t *out, int4 *cand_out, void *d_temp,
                         size_t temp_bytes, uint32_t *d_count, uint32_t *n_out, hipStream_t st);
size_t adapt_temp_bytes(uint32_t n);

}  // namespace mcpt
