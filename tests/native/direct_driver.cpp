// The host loops of mcpt_direct_samples_host / mcpt_direct_fold_host (csrc/mcpt_direct.h: dl::samples_host, dl::fold_host) on heap
// buffers of exactly the documented sizes, for a run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_direct_cpu.py).
// Prints "rc 0 <checksum>" per case; the checksum only keeps the optimiser from dropping the work.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "mcpt_direct.h"

using namespace mcpt;

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float uni(uint32_t &s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

static double run(int64_t n, int32_t N, bool specials) {
    uint32_t s = 12345u + (uint32_t)N;
    std::vector<float> p(3 * n), nf(3 * n), rows((size_t)dl::kLightRow * n * N), q(3 * n * N), ws(3 * n * N), dist(n * N), contrib(3 * n * N), out(3 * n);
    std::vector<uint8_t> live(n * N), vis(n * N);
    for (auto &v : p) v = 2.f * uni(s) - 1.f;
    for (int64_t i = 0; i < n; ++i) nf[3 * i] = 0.f, nf[3 * i + 1] = (i % 3) ? 1.f : -1.f, nf[3 * i + 2] = 0.f;
    for (size_t g = 0; g < (size_t)n * N; ++g) {
        float *r = rows.data() + dl::kLightRow * g;
        r[0] = 2.f * uni(s) - 1.f, r[1] = 2.f + uni(s), r[2] = 2.f * uni(s) - 1.f;
        r[3] = 0.f, r[4] = -1.f, r[5] = 0.f;
        r[6] = 17.f, r[7] = 12.f, r[8] = 4.f;
        r[9] = 0.25f;
        if (specials) {
            const float nan = std::numeric_limits<float>::quiet_NaN();
            switch (g % 6) {
            case 0: r[9] = 0.f; break;                                   // pdf == 0
            case 1: r[4] = 1.f; break;                                   // cl <= 0
            case 2: r[0] = p[3 * (g / N)], r[1] = p[3 * (g / N) + 1] + nf[3 * (g / N) + 1] * dl::kEps, r[2] = p[3 * (g / N) + 2]; break;  // dist == 0 (or nearly)
            case 3: r[3] = nan; break;                                   // NaN light normal
            case 4: r[9] = 1e-38f, r[6] = 1e30f; break;                  // g overflows
            default: break;
            }
        }
    }
    if (specials && n > 0) nf[0] = std::numeric_limits<float>::quiet_NaN();
    dl::samples_host(n, N, p.data(), nf.data(), rows.data(), q.data(), ws.data(), dist.data(), live.data(), contrib.data());
    for (size_t g = 0; g < live.size(); ++g) vis[g] = live[g] && (g % 5 != 0);
    dl::fold_host(n, N, contrib.data(), vis.data(), out.data());
    double sum = 0;
    for (float v : out) sum += std::isfinite(v) ? v : 1.0;
    for (uint8_t v : live) sum += v;
    return sum;
}

int main() {
    const int32_t Ns[] = {1, 3, 4, 32, 4096};
    for (int32_t N : Ns)
        for (int sp = 0; sp < 2; ++sp) std::printf("rc 0 %.6g\n", run(N == 4096 ? 3 : 37, N, sp != 0));
    std::printf("rc 0 %.6g\n", run(0, 4, false));
    return 0;
}
