// The host loop of mcpt_probe_relight_fold_host (csrc/mcpt_probe_relight.h: pr::fold_host) on heap buffers of exactly the documented
// sizes, for a run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_probe_relight_cpu.py).  With a hysteresis of 0 prev is
// a null pointer, which the loop must not read.  Prints "rc 0 <checksum>" per case; the checksum only keeps the optimiser from dropping
// the work.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "mcpt_probe_relight.h"

using namespace mcpt;

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float uni(uint32_t &s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

static double run(int64_t n, int32_t spp, float h, bool specials) {
    uint32_t s = 4321u + (uint32_t)spp;
    std::vector<float> dirs((size_t)3 * n * spp), values((size_t)3 * n * spp), prev, out((size_t)sh::kRow * n);
    for (size_t g = 0; g < (size_t)n * spp; ++g) {
        const float z = 1.f - 2.f * uni(s), r = std::sqrt(std::fmax(0.f, 1.f - z * z)), a = 6.2831853f * uni(s);
        dirs[3 * g] = r * std::cos(a), dirs[3 * g + 1] = r * std::sin(a), dirs[3 * g + 2] = z;
        for (int c = 0; c < 3; ++c) values[3 * g + c] = 4.f * uni(s);
        if (specials) {
            switch (g % 5) {
            case 0: dirs[3 * g] = 0.f, dirs[3 * g + 1] = 0.f, dirs[3 * g + 2] = -1.f; break;  // an axis
            case 1: values[3 * g] = 0.f, values[3 * g + 1] = 0.f, values[3 * g + 2] = 0.f; break;
            case 2: values[3 * g + 1] = std::numeric_limits<float>::infinity(); break;
            case 3: values[3 * g + 2] = std::numeric_limits<float>::quiet_NaN(); break;
            default: break;
            }
        }
    }
    if (h != 0.f) {
        prev.resize((size_t)sh::kRow * n);
        for (auto &v : prev) v = 2.f * uni(s) - 1.f;
    }
    pr::fold_host(n, spp, dirs.data(), values.data(), h, h != 0.f ? prev.data() : nullptr, out.data());
    double sum = 0;
    for (float v : out) sum += std::isfinite(v) ? v : 1.0;
    return sum;
}

int main() {
    const int32_t spps[] = {1, 63, 64, 65, 130};
    const float hs[] = {0.f, 0.5f, std::nextafter(1.f, 0.f)};
    for (int32_t spp : spps)
        for (float h : hs)
            for (int sp = 0; sp < 2; ++sp) std::printf("rc 0 %.6g\n", run(7, spp, h, sp != 0));
    std::printf("rc 0 %.6g\n", run(0, 4, 0.f, false));
    return 0;
}
