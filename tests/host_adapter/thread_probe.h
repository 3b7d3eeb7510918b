// thread_probe.h -- TEST-ONLY, forced in front of every translation unit of the ThreadSanitizer programs (g++ -include): counts the
// std::thread objects the code under test really starts.  The product has no accessor for "how many host threads did this pass use" (and
// shall not grow one for a test), and the thresholds that decide it live in host_pack.h / ald_sink.cpp; a case that quietly fell back to
// one thread would check nothing.  So `std::thread` is spelled std::probed_thread here: the same thread, plus two counters in the
// STARTING thread's own storage --
//   started : threads this thread has started
//   peak    : most threads this thread had started and not yet joined (HostBatch::run_threads starts nthr - 1 and joins them: the width
//             of the widest pass a call made is peak + 1)
// Every standard header the project uses is included before the macro, so that the library's own text never sees it.
#pragma once
#include <thread>
#include <mutex>
#include <condition_variable>
#include <atomic>
#include <chrono>
#include <future>
#include <memory>
#include <string>
#include <vector>
#include <deque>
#include <map>
#include <set>
#include <unordered_map>
#include <algorithm>
#include <numeric>
#include <iterator>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <new>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime.h>
#endif

struct thread_probe_counts { long started = 0, live = 0, peak = 0; };
inline thread_probe_counts &thread_probe() { static thread_local thread_probe_counts c; return c; }
inline void thread_probe_reset() { thread_probe() = thread_probe_counts(); }

namespace std {
class probed_thread : public thread {
public:
    probed_thread() noexcept {}
    template<class F, class... A, class = typename enable_if<!is_same<typename decay<F>::type, probed_thread>::value>::type>
    explicit probed_thread(F &&f, A &&... a) : thread(std::forward<F>(f), std::forward<A>(a)...)
    {
        thread_probe_counts &c = thread_probe(); c.started++; if(++c.live > c.peak) c.peak = c.live;
    }
    probed_thread(probed_thread &&) = default;
    probed_thread &operator=(probed_thread &&) = default;
    void join() { thread::join(); thread_probe().live--; }
};
}
#define thread probed_thread
