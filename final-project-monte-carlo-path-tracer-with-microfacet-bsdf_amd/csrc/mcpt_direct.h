/*
 * mcpt_direct.h -- the rule of the sampled direct term (include/mcpt.h: mcpt_query_direct and its host forms): the geometry of one
 * light sample at a Lambertian point, the visibility window of its shadow ray, and the fold of a point's samples.
 *
 * Like csrc/mcpt_sh.h: every function is callable from the host and from the device, both compilations run with -ffp-contract=off,
 * float32 in the written order, and only + - * /, sqrtf and fabs are used.  A three-term dot product is a.x * b.x + (a.y * b.y + a.z * b.z),
 * norm and normalized are those of csrc/mcpt_device.h.  The light sample itself (sample_light, csrc/mcpt_kernels.hip) and the Philox
 * block (rng_block, csrc/mcpt_device.h) are not restated here.  tests/test_direct_cpu.py checks the host loops against the numpy
 * restatement of tests/direct_cases.py, tests/test_gpu_direct.py the device against the host composition, bit for bit.
 *
 * At the end, host only: the cut of a staged query into launches (piece_cut, for_each_piece), which the direct term shares with the
 * probe depth query.
 */
#ifndef MCPT_DIRECT_H
#define MCPT_DIRECT_H

#include "mcpt_sh.h"

namespace mcpt {
namespace dl {

constexpr int32_t kMaxSamples = 4096;  // light samples per point and call
constexpr int32_t kLightRow = 10;      // floats of a light sample: x_l, n_l, emit, pdf (mcpt_debug_scene kind 0)
constexpr float kEps = 1e-4f;          // EPSILON (kEps of csrc/mcpt_internal.h)
constexpr float kPi = 3.141592653589793f;
constexpr float kFltMax = 3.4028234663852886e38f;

MCPT_SH float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }

// One light sample `row` seen from the point p with unit normal nf, as one of N: the origin q and unit direction ws of its shadow ray,
// the distance dist to the sample, and contrib[c] = (emit[c] * g) / N.  Returns whether the sample is live; a sample that is not has
// contrib 0 and traces no ray (q, ws and dist are still what the rule gives).
MCPT_SH bool sample_geometry(const float p[3], const float nf[3], const float row[kLightRow], int32_t N, float q[3], float ws[3], float &dist,
                             float contrib[3]) {
    q[0] = p[0] + nf[0] * kEps;  // Scene.cpp:114
    q[1] = p[1] + nf[1] * kEps;
    q[2] = p[2] + nf[2] * kEps;
    const float w[3] = {row[0] - q[0], row[1] - q[1], row[2] - q[2]};
    const float z = dot3(w, w);
    dist = sqrtf(z);
    ws[0] = w[0], ws[1] = w[1], ws[2] = w[2];
    if (z > 0.0f) {  // (Eigen normalized(): unchanged when the squared norm is 0)
        const float l = sqrtf(z);
        ws[0] = w[0] / l;
        ws[1] = w[1] / l;
        ws[2] = w[2] / l;
    }
    const float mws[3] = {-ws[0], -ws[1], -ws[2]};
    const float cs = dot3(ws, nf), cl = dot3(mws, row + 3);
    const float g = ((cs * cl) / (dist * dist)) / row[9];
    const bool live = cs > 0.f && cl > 0.f && g <= kFltMax;  // (a NaN fails; a zero distance has cs == 0)
    for (int c = 0; c < 3; ++c) contrib[c] = live ? (row[6 + c] * g) / (float)N : 0.f;
    return live;
}

// Scene.cpp:72-75: the sample is seen iff the closest hit of its shadow ray lies within EPSILON of the sample's distance.
MCPT_SH bool in_window(double t, float dist) { return fabs(t - (double)dist) < (double)kEps; }

// One sample folded into a point's sum, and the sum's end.
MCPT_SH void fold_sample(const float contrib[3], float acc[3]) {
    acc[0] = acc[0] + contrib[0];
    acc[1] = acc[1] + contrib[1];
    acc[2] = acc[2] + contrib[2];
}
MCPT_SH void fold_end(const float acc[3], float out[3]) {
    out[0] = acc[0] / kPi;
    out[1] = acc[1] / kPi;
    out[2] = acc[2] / kPi;
}

// The host loops of mcpt_direct_samples_host and mcpt_direct_fold_host after their argument checks (csrc/mcpt_probes.hip); a stand-alone
// program runs them under the sanitizers (tests/native/direct_driver.cpp).
static inline void samples_host(int64_t n, int32_t N, const float *points, const float *normals, const float *light_rows, float *q_out, float *ws_out,
                                float *dist_out, uint8_t *live_out, float *contrib_out) {
    for (int64_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < N; ++j) {
            const size_t g = (size_t)i * (size_t)N + (size_t)j;
            live_out[g] = sample_geometry(points + 3 * i, normals + 3 * i, light_rows + kLightRow * g, N, q_out + 3 * g, ws_out + 3 * g, dist_out[g],
                                          contrib_out + 3 * g)
                              ? 1
                              : 0;
        }
}

static inline void fold_host(int64_t n, int32_t N, const float *contrib, const uint8_t *visible, float *out) {
    for (int64_t i = 0; i < n; ++i) {
        float acc[3] = {0.f, 0.f, 0.f};
        for (int32_t j = 0; j < N; ++j) {
            const size_t g = (size_t)i * (size_t)N + (size_t)j;
            if (visible[g]) fold_sample(contrib + 3 * g, acc);
        }
        fold_end(acc, out + 3 * i);
    }
}

}  // namespace dl

// The cut of a staged query (mcpt_query_probe_depth, mcpt_query_direct, the direct term of the lit pass) into launches: n items of
// `samples` samples each through a staging of `capacity` samples.  A launch holds whole items when an item's samples fit the staging,
// else a run of one item's samples, whole blocks of `block` but for the item's last run (capacity >= block).  The one place that says
// so: the staging is sized by staged(), the loops are for_each_piece's.  tests/native/piece_cut_driver.cpp walks it.
struct PieceCut {
    uint64_t per, smax;  // items per launch, samples of an item per launch
    uint64_t staged() const { return per * smax; }
};

static inline PieceCut piece_cut(uint64_t n, uint64_t samples, uint64_t capacity, uint64_t block) {
    if (samples <= capacity) return PieceCut{n < capacity / samples ? n : capacity / samples, samples};
    return PieceCut{1, capacity / block * block};
}

// f(i0, m, s0, sc) for every launch, items outermost and an item's runs in sample order: samples s0 .. s0 + sc - 1 of items i0 .. i0 + m - 1.
// It returns an mcpt status; the first that is not 0 ends the walk and is returned.
template <class F>
int for_each_piece(const PieceCut &c, uint64_t n, uint64_t samples, F &&f) {
    for (uint64_t i0 = 0; i0 < n; i0 += c.per)
        for (uint64_t s0 = 0; s0 < samples; s0 += c.smax) {
            const uint64_t m = c.per < n - i0 ? c.per : n - i0, sc = c.smax < samples - s0 ? c.smax : samples - s0;
            if (const int rc = f((uint32_t)i0, (uint32_t)m, (uint32_t)s0, (uint32_t)sc)) return rc;
        }
    return 0;
}

}  // namespace mcpt

#endif /* MCPT_DIRECT_H */
