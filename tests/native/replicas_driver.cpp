// The replica fan-out of the group calls (csrc/mcpt_replicas.h: on_replicas) without a GPU, for a run under AddressSanitizer +
// UndefinedBehaviorSanitizer and, as a second build, under ThreadSanitizer (tests/test_replicas_cpu.py).  For n in 1..8 and every subset
// of failing replicas: apply ran once on every replica; undo ran once on exactly the replicas whose apply succeeded, and not at all when
// none failed; the failure reported is the lowest failing replica's, with its code and its thread's text; every worker thread was joined.
// Prints "ok <cases>".
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mcpt_replicas.h"

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s: n %d failing mask 0x%x\n", #cond, n, mask);        \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

// The error text of a thread, as mcpt::g_err is.  Its destructor runs when the thread ends, and join() returns after that: with every
// worker joined, as many have died as were born.
static std::atomic<int> g_born{0}, g_died{0};
struct ThreadError {
    std::string text;
    ThreadError() { g_born++; }
    ~ThreadError() { g_died++; }
};
static thread_local ThreadError t_err;

static void one_case(int n, unsigned mask) {
    std::atomic<int> applied[8], undone[8];
    for (int i = 0; i < 8; ++i) applied[i] = 0, undone[i] = 0;
    const int born0 = g_born, died0 = g_died;
    const mcpt::ReplicaFailure f = mcpt::on_replicas(
        n,
        [&](int i) {
            applied[i]++;
            t_err.text = "apply " + std::to_string(i) + " of " + std::to_string(n);  // (set whether it fails or not: a stale text must not be reported)
            return (mask >> i) & 1u ? 100 + i : 0;
        },
        [&](int i) {
            undone[i]++;
            t_err.text = "undo " + std::to_string(i);
            return (i & 1) ? 7 : 0;  // (what undo returns is not looked at)
        },
        []() { return t_err.text.c_str(); });
    int lowest = -1;
    for (int i = n - 1; i >= 0; --i)
        if ((mask >> i) & 1u) lowest = i;
    for (int i = 0; i < n; ++i) {
        REQUIRE(applied[i] == 1);
        REQUIRE(undone[i] == (mask != 0 && !((mask >> i) & 1u) ? 1 : 0));
    }
    REQUIRE(f.index == lowest);
    if (lowest >= 0) {
        REQUIRE(f.code == 100 + lowest);
        REQUIRE(f.message == "apply " + std::to_string(lowest) + " of " + std::to_string(n));
    } else {
        REQUIRE(f.code == 0 && f.message.empty());
    }
    REQUIRE(g_born - born0 == g_died - died0);  // every worker that started has ended: all were joined
    const int succeeded = n - __builtin_popcount(mask);
    REQUIRE(g_born - born0 == (n - 1) + (mask != 0 && succeeded > 0 ? succeeded - 1 : 0));  // replica 0 of each round runs on the caller's thread
}

int main() {
    (void)t_err.text.size();  // the caller's own instance, born before the first count is taken
    int cases = 0;
    for (int n = 1; n <= 8; ++n)
        for (unsigned mask = 0; mask < (1u << n); ++mask, ++cases) one_case(n, mask);
    std::printf("ok %d\n", cases);
    return 0;
}
