// tsan_control_race.cc -- TEST-ONLY liveness control of tests/test_host_threads_cpu.py: two threads increment one plain long without a
// lock.  Built with the flags of the ThreadSanitizer programs it MUST end non-zero with a "data race" report; where it does not, the
// sanitizer does nothing in this environment and a clean run of the real programs would prove nothing.
#include <cstdio>
#include <thread>

static long counter = 0;

int main()
{
    auto work = [] { for(int i = 0; i < 100000; i++) counter++; };
    std::thread a(work), b(work);
    a.join(); b.join();
    printf("counter %ld\n", counter);
    return 0;
}
