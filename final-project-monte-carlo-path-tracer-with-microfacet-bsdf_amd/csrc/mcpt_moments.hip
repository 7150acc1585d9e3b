// The variance of an accumulated frame from its temporal luminance moments (include/mcpt.h: mcpt_moments_variance, step 5b of a moments
// sequence's frame); csrc/mcpt_moments.h has the arithmetic, shared with the CPU build the tests compare against.
//   k_moments_variance  16 x 16 pixel blocks, one pixel per lane.  A lane on the temporal branch reads its own moments, length and flag and
//                       is done: no window work.  A lane on the spatial branch (a short or clamped history) walks its (2r + 1)^2 window, at
//                       most 81 taps, each the second half of an AOV record and the 8-byte moments, read straight from global memory as
//                       k_dn_atrous reads its records: neighbouring lanes' windows overlap, so the lines are shared in L1 / L2, and after
//                       the first frames of a sequence only disoccluded or clamped pixels take this branch at all.  No LDS, no scratch, no
//                       double precision, no atomics; every store a plain vector store.
#include <hip/hip_runtime.h>

#include "mcpt_moments.h"

namespace mcpt {

namespace {

constexpr int kTile = 16;

__global__ __launch_bounds__(kTile *kTile) void k_moments_variance(int W, int H, mo::Opts o, const float *__restrict__ moments, const float *__restrict__ len,
                                                                  const uint8_t *__restrict__ flags, const float *__restrict__ aov, float *__restrict__ out) {
    const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= W || y >= H) return;
    out[(size_t)y * W + x] = mo::variance_pixel(W, H, x, y, moments, len, flags, aov, o);
}

}  // namespace

void launch_moments_variance(int W, int H, const mo::Opts &o, const float *moments, const float *len, const uint8_t *flags, const float *aov, float *out,
                             hipStream_t st) {
    hipLaunchKernelGGL(k_moments_variance, dim3((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), dim3(kTile, kTile), 0, st, W, H, o, moments, len, flags,
                       aov, out);
}

}  // namespace mcpt
