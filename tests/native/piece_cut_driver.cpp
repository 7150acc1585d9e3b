// The cut of a staged query into launches (csrc/mcpt_direct.h: piece_cut, for_each_piece) walked the way mcpt_query_probe_depth (block 64)
// and the direct term (block 1) walk it, for a run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_piece_cut_cpu.py).
// Every property is checked per launch against a cursor (next item, next sample), so a walk costs its launches, not its samples.
// Prints "<name> <n> <samples> <launches>" for the launch counts the GPU tests pin at capacity 64, then "ok <walks>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "mcpt_direct.h"

using namespace mcpt;

#define REQUIRE(cond)                                                                                                              \
    do {                                                                                                                           \
        if (!(cond)) {                                                                                                             \
            std::printf("FAILED %s: n %llu samples %llu capacity %llu block %llu\n", #cond, (unsigned long long)n,                 \
                        (unsigned long long)samples, (unsigned long long)capacity, (unsigned long long)block);                     \
            std::exit(1);                                                                                                          \
        }                                                                                                                          \
    } while (0)

// One walk -> its launches.
static uint64_t walk(uint64_t n, uint64_t samples, uint64_t capacity, uint64_t block) {
    const PieceCut cut = piece_cut(n, samples, capacity, block);
    REQUIRE(cut.per >= 1 && cut.smax >= 1 && cut.staged() <= capacity);
    uint64_t item = 0, sample = 0, launches = 0;  // the cursor: every pair before (item, sample), items first, has been visited once
    const int rc = for_each_piece(cut, n, samples, [&](uint32_t i0, uint32_t m, uint32_t s0, uint32_t sc) -> int {
        REQUIRE(i0 == item && s0 == sample);              // in order, nothing skipped, nothing twice
        REQUIRE(m >= 1 && sc >= 1 && item + m <= n && sample + sc <= samples);
        REQUIRE((uint64_t)m * sc <= cut.staged());        // no launch stages more than the staging holds (<= capacity, above)
        REQUIRE(m == 1 || (s0 == 0 && sc == samples));   // several items in a launch: whole items
        REQUIRE(sample + sc == samples || sc % block == 0);  // a run that is not an item's last: whole blocks
        sample += sc;
        if (sample == samples) item += m, sample = 0;
        launches++;
        return 0;
    });
    REQUIRE(rc == 0 && item == n && sample == 0);
    REQUIRE(launches == (n + cut.per - 1) / cut.per * ((samples + cut.smax - 1) / cut.smax));
    return launches;
}

int main() {
    const uint64_t capacities[3] = {64, 128, 1u << 20}, blocks[2] = {1, 64};
    uint64_t walks = 0;
    for (uint64_t capacity : capacities)
        for (uint64_t block : blocks)
            for (uint64_t n = 1; n <= 200; ++n) {
                for (uint64_t samples = 1; samples <= 200; ++samples) walk(n, samples, capacity, block);
                walk(n, 4096, capacity, block);
                walks += 201;
            }
    // an error from the callback ends the walk and is returned
    int calls = 0;
    if (for_each_piece(piece_cut(10, 5, 64, 1), 10, 5, [&](uint32_t, uint32_t, uint32_t, uint32_t) { return ++calls == 1 ? 7 : 0; }) != 7 || calls != 1) return 1;
    const uint64_t depth[4][2] = {{65, 5}, {65, 64}, {65, 70}, {3, 130}}, direct[3][2] = {{101, 100}, {37, 64}, {37, 65}};
    for (const auto &c : depth) std::printf("depth %llu %llu %llu\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)walk(c[0], c[1], 64, 64));
    for (const auto &c : direct) std::printf("direct %llu %llu %llu\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)walk(c[0], c[1], 64, 1));
    const uint64_t per_launch[2] = {3, 32};  // 21 and 2 points fit a launch
    for (uint64_t samples : per_launch)
        for (uint64_t n = 1; n <= 200; ++n) std::printf("direct %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)samples, (unsigned long long)walk(n, samples, 64, 1));
    std::printf("ok %llu\n", (unsigned long long)walks);
    return 0;
}
