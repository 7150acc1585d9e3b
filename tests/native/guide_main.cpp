// Stand-alone run of the host build of tp::history_len_pixel (csrc/mcpt_temporal.h) for a sanitizer build:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I csrc guide_main.cpp
// Every array is a heap allocation of exactly its size, so a read or write one element past a plane is an AddressSanitizer error.  The
// inputs are those of tests/native/history_main.cpp: the three frame shapes of the tests, motions that are fractional, huge, infinite and
// NaN, NaN colours and normals, the normal test on and off.  Each run also checks the function's contract against tp::accumulate_pixel_ex:
// the same length on every pixel whose new colour is finite.  Prints a checksum per run; exit status 0 unless a sanitizer stops it or the
// contract fails.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcpt_temporal.h"

using namespace mcpt;

namespace {

uint32_t state = 54321u;
float rnd() {  // [0, 1)
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) * (1.0f / 16777216.0f);
}

int run(int W, int H, int normal_test, int color_clamp) {
    const size_t n = (size_t)W * H;
    std::vector<float> color(n * 3), variance(n), motion(n * 4), normal(n * 3), prev_color(n * 3), prev_variance(n), prev_depth(n), prev_len(n),
        prev_normal(n * 3), out_color(n * 3), out_variance(n), out_len(n), len(n);
    const float odd[] = {-1e30f, 1e30f, INFINITY, -INFINITY, NAN, -0.5f, 0.5f, (float)W, -(float)W - 0.5f, (float)H + 0.25f};
    for (size_t m = 0; m < n; ++m) {
        for (int c = 0; c < 3; ++c) {
            color[m * 3 + c] = rnd() * 2.0f;
            prev_color[m * 3 + c] = rnd() * 2.0f;
            normal[m * 3 + c] = rnd() * 2.0f - 1.0f;
            prev_normal[m * 3 + c] = normal[m * 3 + c] + (rnd() - 0.5f) * 0.5f;
        }
        if (rnd() < 0.1f) color[m * 3 + (int)(rnd() * 3.0f)] = rnd() < 0.5f ? NAN : INFINITY;
        if (rnd() < 0.1f) prev_color[m * 3 + (int)(rnd() * 3.0f)] = NAN;
        if (rnd() < 0.1f) normal[m * 3 + (int)(rnd() * 3.0f)] = NAN;
        if (rnd() < 0.1f) prev_normal[m * 3 + (int)(rnd() * 3.0f)] = NAN;
        variance[m] = rnd() * 0.1f;
        prev_variance[m] = rnd() * 0.05f;
        prev_depth[m] = 5.0f + 0.002f * (float)(m % W) + 0.003f * (float)(m / W);
        prev_len[m] = (float)(int)(rnd() * 40.0f);
        motion[m * 4] = rnd() * 6.0f - 3.0f;
        motion[m * 4 + 1] = rnd() * 6.0f - 3.0f;
        if (rnd() < 0.3f) motion[m * 4] = odd[(int)(rnd() * 10.0f)];
        if (rnd() < 0.3f) motion[m * 4 + 1] = odd[(int)(rnd() * 10.0f)];
        motion[m * 4 + 2] = prev_depth[m];
        motion[m * 4 + 3] = rnd() < 0.1f ? 0.0f : 1.0f;
    }
    mcpt_temporal_opts to;
    mcpt_history_opts hopts;
    std::memset(&to, 0, sizeof to);
    std::memset(&hopts, 0, sizeof hopts);
    hopts.normal_test = normal_test;
    hopts.color_clamp = color_clamp;
    tp::Opts o;
    tp::HistOpts ho;
    if (tp::resolve_opts(to, o) != 0 || tp::resolve_history_opts(hopts, ho) != 0) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) {
            len[(size_t)j * W + i] = tp::history_len_pixel(W, H, i, j, motion.data(), normal_test ? normal.data() : nullptr, 3, prev_color.data(),
                                                           prev_depth.data(), prev_len.data(), normal_test ? prev_normal.data() : nullptr, o, ho);
            tp::accumulate_pixel_ex(W, H, i, j, color.data(), variance.data(), motion.data(), normal_test ? normal.data() : nullptr, 3, prev_color.data(),
                                    prev_variance.data(), prev_depth.data(), prev_len.data(), normal_test ? prev_normal.data() : nullptr, o, ho,
                                    out_color.data(), out_variance.data(), out_len.data(), nullptr);
        }
    uint32_t sum = 0, bits;
    size_t longer = 0, differ = 0;
    for (size_t m = 0; m < n; ++m) {
        std::memcpy(&bits, &len[m], 4);
        sum = sum * 31u + bits;
        longer += len[m] > 1.0f;
        const bool finite = std::isfinite(color[m * 3]) && std::isfinite(color[m * 3 + 1]) && std::isfinite(color[m * 3 + 2]);
        if (finite && len[m] != out_len[m]) {
            std::printf("pixel %zu: guide %g, blend %g\n", m, len[m], out_len[m]);
            return 1;
        }
        differ += len[m] != out_len[m];
    }
    std::printf("%2d x %2d normal_test %d color_clamp %d: checksum %08x, %zu pixels with history, %zu differ from the blend (colour not finite)\n", W, H,
                normal_test, color_clamp, sum, longer, differ);
    return 0;
}

}  // namespace

int main() {
    const int shapes[3][2] = {{1, 1}, {5, 3}, {33, 17}};
    for (const auto &s : shapes)
        for (int sw = 0; sw < 4; ++sw)
            if (run(s[0], s[1], sw & 1, sw >> 1) != 0) return 1;
    std::printf("ok\n");
    return 0;
}
