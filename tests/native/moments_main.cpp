// Stand-alone run of the host build of tp::accumulate_pixel_moments (csrc/mcpt_temporal.h) and mo::variance_pixel (csrc/mcpt_moments.h) for a
// sanitizer build:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I csrc moments_main.cpp
// Every array is a heap allocation of exactly its size, so a read or write one element past a plane is an AddressSanitizer error.  The
// inputs cover what the index arithmetic depends on: the frame shapes of the tests (image edges on every side of a window of radius up
// to 4, a frame that crosses 16 x 16 tile borders), motions that are fractional, huge, infinite and NaN, history holes, NaN colours, stored
// moments that are not finite, clamped pixels, coverage seams and NaN depths, the four combinations of the switches, min_len 2 and 4,
// radius 1, 3 and 4.  Prints a checksum per run; exit status 0 unless a sanitizer stops it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcpt_moments.h"

using namespace mcpt;

namespace {

uint32_t state = 2468u;
float rnd() {  // [0, 1)
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) * (1.0f / 16777216.0f);
}

int run(int W, int H, int normal_test, int color_clamp, int min_len, int radius) {
    const size_t n = (size_t)W * H;
    std::vector<float> color(n * 3), motion(n * 4), normal(n * 3), prev_color(n * 3), prev_depth(n), prev_len(n), prev_normal(n * 3), prev_moments(n * 2),
        out_color(n * 3), out_len(n), out_moments(n * 2), aov(n * 8), var(n);
    std::vector<uint8_t> flags(n);
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
        prev_moments[m * 2] = rnd();
        prev_moments[m * 2 + 1] = prev_moments[m * 2] * prev_moments[m * 2] + rnd() * 0.1f;
        if (rnd() < 0.1f) prev_moments[m * 2 + (rnd() < 0.5f)] = rnd() < 0.5f ? NAN : INFINITY;
        prev_depth[m] = 5.0f + 0.002f * (float)(m % W) + 0.003f * (float)(m / W);
        prev_len[m] = (float)(int)(rnd() * 12.0f);  // (holes of length 0 among them)
        motion[m * 4] = rnd() * 6.0f - 3.0f;
        motion[m * 4 + 1] = rnd() * 6.0f - 3.0f;
        if (rnd() < 0.3f) motion[m * 4] = odd[(int)(rnd() * 10.0f)];
        if (rnd() < 0.3f) motion[m * 4 + 1] = odd[(int)(rnd() * 10.0f)];
        motion[m * 4 + 2] = prev_depth[m] * (rnd() < 0.1f ? 2.0f : 1.0f);  // (some taps fail the depth test)
        motion[m * 4 + 3] = rnd() < 0.1f ? 0.0f : 1.0f;
        float *a = &aov[m * 8];
        a[0] = a[1] = a[2] = 0.5f;
        for (int c = 0; c < 3; ++c) a[3 + c] = normal[m * 3 + c];
        a[6] = rnd() < 0.05f ? NAN : prev_depth[m] + ((m % W) * 2 > (size_t)W ? 3.0f : 0.0f);
        a[7] = rnd() < 0.15f ? 0.0f : 1.0f;
    }
    mcpt_temporal_opts to;
    mcpt_history_opts hopts;
    mcpt_moments_opts mopts;
    std::memset(&to, 0, sizeof to);
    std::memset(&hopts, 0, sizeof hopts);
    std::memset(&mopts, 0, sizeof mopts);
    hopts.normal_test = normal_test;
    hopts.color_clamp = color_clamp;
    mopts.enabled = 1;
    mopts.min_len = min_len;
    mopts.radius = radius;
    tp::Opts o;
    tp::HistOpts ho;
    mo::Opts mo_o;
    if (tp::resolve_opts(to, o) != 0 || tp::resolve_history_opts(hopts, ho) != 0 || mo::resolve_opts(mopts, mo_o) != 0) return 1;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            tp::accumulate_pixel_moments(W, H, i, j, color.data(), motion.data(), normal_test ? normal.data() : nullptr, 3, prev_color.data(),
                                         prev_depth.data(), prev_len.data(), normal_test ? prev_normal.data() : nullptr, prev_moments.data(), o, ho,
                                         out_color.data(), out_len.data(), flags.data(), out_moments.data());
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i)
            var[(size_t)j * W + i] = mo::variance_pixel(W, H, i, j, out_moments.data(), out_len.data(), color_clamp ? flags.data() : nullptr, aov.data(), mo_o);
    uint32_t sum = 0, bits;
    size_t took = 0, spatial = 0, notfinite = 0;
    for (size_t m = 0; m < n; ++m) {
        for (int c = 0; c < 2; ++c) {
            std::memcpy(&bits, &out_moments[m * 2 + c], 4);
            sum = sum * 31u + bits;
        }
        std::memcpy(&bits, &var[m], 4);
        sum = sum * 31u + bits;
        took += out_len[m] > 1.0f;
        spatial += !(out_len[m] >= (float)min_len) || (flags[m] & 2);
        notfinite += !(var[m] - var[m] == 0.0f);
    }
    std::printf("%2d x %2d normal_test %d color_clamp %d min_len %d radius %d: checksum %08x, %zu pixels took history, %zu spatial, %zu not finite\n", W, H,
                normal_test, color_clamp, min_len, radius, sum, took, spatial, notfinite);
    return 0;
}

}  // namespace

int main() {
    const int shapes[4][2] = {{1, 1}, {8, 8}, {17, 13}, {40, 24}};
    for (const auto &s : shapes)
        for (int sw = 0; sw < 4; ++sw)
            if (run(s[0], s[1], sw & 1, sw >> 1, (sw & 1) ? 2 : 4, sw == 0 ? 4 : ((sw >> 1) ? 1 : 3)) != 0) return 1;
    std::printf("ok\n");
    return 0;
}
