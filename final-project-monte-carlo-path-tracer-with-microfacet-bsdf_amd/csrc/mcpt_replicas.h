// One call on every replica of a group and the way back when a replica fails.  Host code that includes neither HIP nor mcpt_group:
// csrc/mcpt_multi.hip wraps it, tests/native/replicas_driver.cpp runs it under the sanitizers.
#pragma once
#include <string>
#include <thread>
#include <vector>

namespace mcpt {

struct ReplicaFailure {
    int index = -1;  // the lowest replica whose apply failed; -1: none did
    int code = 0;    // what its apply returned,
    std::string message;  // and its thread's error text right after
};

// apply(i) for every i in [0, n), one host thread per replica (replica 0 on the caller's); a result other than 0 is a failure, and
// last_error() is read on the thread that got it.  If any replica failed, undo(i) then runs the same way on the replicas whose apply
// succeeded, so that the group stays one scene (what undo returns is not looked at).  Every thread is joined before the return.
// static: every translation unit gets its own; nothing enters a library's symbol table.
template <typename Apply, typename Undo, typename LastError>
static ReplicaFailure on_replicas(int n, Apply apply, Undo undo, LastError last_error) {
    std::vector<int> rc((size_t)n, 0);
    std::vector<std::string> err((size_t)n);
    const auto run = [](const std::vector<int> &which, auto work) {
        std::vector<std::thread> th;
        for (size_t k = 1; k < which.size(); ++k) th.emplace_back(work, which[k]);
        if (!which.empty()) work(which[0]);
        for (std::thread &t : th) t.join();
    };
    std::vector<int> all, done;
    for (int i = 0; i < n; ++i) all.push_back(i);
    run(all, [&](int i) {
        rc[(size_t)i] = apply(i);
        if (rc[(size_t)i] != 0) err[(size_t)i] = last_error();
    });
    ReplicaFailure f;
    for (int i = 0; i < n; ++i) {
        if (rc[(size_t)i] == 0) done.push_back(i);
        else if (f.index < 0) f.index = i;
    }
    if (f.index < 0) return f;
    f.code = rc[(size_t)f.index];
    f.message = err[(size_t)f.index];
    run(done, [&](int i) { (void)undo(i); });
    return f;
}

}  // namespace mcpt
