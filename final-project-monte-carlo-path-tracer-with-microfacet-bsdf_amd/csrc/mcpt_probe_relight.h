/*
 * mcpt_probe_relight.h -- the rule of relighting a probe volume from itself (include/mcpt.h: mcpt_probe_volume_relight and its host form
 * mcpt_probe_relight_fold_host): one term of the projection fold of a probe's samples, and the hysteresis blend with the previous
 * coefficients.  The basis is sh::sh9_basis of csrc/mcpt_sh.h.
 *
 * Like csrc/mcpt_sh.h: every function is callable from the host and from the device, both compilations run with -ffp-contract=off,
 * float32 in the written order, no FMA.  k_probe_relight_fold (csrc/mcpt_probes.hip) and the host loop below call these functions and
 * nothing else decides a coefficient.  tests/test_probe_relight_cpu.py checks the host loop against a numpy restatement of the header's
 * text, tests/test_gpu_probe_relight.py the device against the restatement of a whole update, bit for bit; a stand-alone program runs
 * the host loop under the sanitizers (tests/native/probe_relight_driver.cpp).
 */
#ifndef MCPT_PROBE_RELIGHT_H
#define MCPT_PROBE_RELIGHT_H

#include "mcpt_sh.h"

namespace mcpt {
namespace pr {

// The weight of a sample with direction d in coefficient j: the basis value over the uniform-sphere pdf.
MCPT_SH float weight(float Yj) { return sh::kFourPi * Yj; }

// One sample folded into a coefficient's sum: acc + (v * w) / (float)spp, mcpt_query_probes' projection with spp_total = spp.
MCPT_SH float fold_term(float acc, float v, float w, float fn) { return acc + (v * w) / fn; }

// The coefficient a probe ends with: the fresh projection, or with a hysteresis h > 0 the share h of the previous coefficient kept.
MCPT_SH float blend(float h, float prev, float fresh) { return h == 0.0f ? fresh : h * prev + (1.0f - h) * fresh; }

// The host loop of mcpt_probe_relight_fold_host after its argument checks: dirs and values n*spp*3, probe-major in sample order;
// prev (n*27) is read only when h != 0.
static inline void fold_host(int64_t n, int32_t spp, const float *dirs, const float *values, float h, const float *prev, float *out) {
    const float fn = (float)spp;
    for (int64_t i = 0; i < n; ++i) {
        float acc[sh::kRow];
        for (int32_t q = 0; q < sh::kRow; ++q) acc[q] = 0.f;
        for (int32_t k = 0; k < spp; ++k) {
            const size_t g = ((size_t)i * (size_t)spp + (size_t)k) * 3;
            float Y[sh::kCoef];
            sh::sh9_basis(dirs + g, Y);
            for (int32_t j = 0; j < sh::kCoef; ++j) {
                const float w = weight(Y[j]);
                for (int32_t c = 0; c < 3; ++c) acc[3 * j + c] = fold_term(acc[3 * j + c], values[g + c], w, fn);
            }
        }
        for (int32_t q = 0; q < sh::kRow; ++q) out[sh::kRow * i + q] = blend(h, h == 0.0f ? 0.f : prev[sh::kRow * i + q], acc[q]);
    }
}

}  // namespace pr
}  // namespace mcpt

#endif /* MCPT_PROBE_RELIGHT_H */
