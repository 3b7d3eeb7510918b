// dispatch_test.cc -- exercises aletsch_amd/host/gpu_dispatch.hpp (queue + flusher over the C ABI) with the mock types of
// adapter_test.cc.  stdin: "N T B S D" (graphs, submitting threads, graphs per batch, slots per device, device slots -- all on HIP
// device 0: D > 1 runs the several-devices-in-one-process form with D GPU threads), then N graphs in adapter_test's format.
// Thread t submits graphs t, t + T, ...; sample id of graph g = g % 3.  Prints the merged sink.  Driven by tests/test_gpu_adapter.py.
#include "mock_types.h"

int main()
{
    int N, T, B, S, D;
    if(scanf("%d %d %d %d %d", &N, &T, &B, &S, &D) != 5) return 2;
    std::vector<mock_graph> gs((size_t)N); std::vector<mock_hyper_set> hs((size_t)N); mock_parameters cfg;
    for(int n = 0; n < N; n++) if(!read_mock_graph(stdin, gs[(size_t)n], hs[(size_t)n])) return 2;
    ald_tset *tm = nullptr;
    if(ald_tset_create(0.8, &tm) != ALD_OK) return 3;
    try {
        aletsch::gpu_assembly_queue<mock_graph, mock_hyper_set, mock_parameters> q(cfg, tm, false, std::vector<int>((size_t)D, 0), B, S);
        std::vector<std::thread> th;
        for(int t = 0; t < T; t++) th.emplace_back([&, t] { for(int n = t; n < N; n += T) q.submit(gs[(size_t)n], hs[(size_t)n], n % 3); });
        for(auto &x : th) x.join();
        q.drain();
        printf("submitted %ld failed %ld batches %ld\n", q.submitted(), q.failed_graphs(), q.batches());
        // a second round through the same queue (slots are reused after a drain)
        q.drain();
    } catch(const std::exception &e) { printf("EXCEPTION %s\n", e.what()); return 1; }
    int64_t n = 0, ne = 0, ns = 0;
    ald_tset_size(tm, &n, &ne, &ns);
    std::vector<uint64_t> h((size_t)n + 1); std::vector<int32_t> cnt((size_t)n + 1), c1((size_t)n + 1), c2((size_t)n + 1), lr(2 * (size_t)ne + 2), ssid((size_t)ns + 1), sc1((size_t)ns + 1);
    std::vector<char> st((size_t)n + 1); std::vector<double> cov((size_t)n + 1), cov2((size_t)n + 1), conf((size_t)n + 1), abd((size_t)n + 1), scov2((size_t)ns + 1), sconf((size_t)ns + 1), sabd((size_t)ns + 1);
    std::vector<int64_t> tid((size_t)n + 1), eo((size_t)n + 2), so((size_t)n + 2);
    if(ald_tset_export(tm, h.data(), cnt.data(), st.data(), cov.data(), cov2.data(), conf.data(), abd.data(), c1.data(), c2.data(), tid.data(), eo.data(), lr.data(),
                       so.data(), ssid.data(), scov2.data(), sconf.data(), sabd.data(), sc1.data()) != ALD_OK) return 4;
    for(int64_t i = 0; i < n; i++) {
        printf("%llu %d %c %.17g %.17g %.17g %.17g %d %d %lld :", (unsigned long long)h[(size_t)i], cnt[(size_t)i], st[(size_t)i], cov[(size_t)i], cov2[(size_t)i], conf[(size_t)i], abd[(size_t)i], c1[(size_t)i], c2[(size_t)i], (long long)tid[(size_t)i]);
        for(int64_t k = eo[(size_t)i]; k < eo[(size_t)i + 1]; k++) printf(" %d-%d", lr[2 * (size_t)k], lr[2 * (size_t)k + 1]);
        printf(" :");
        for(int64_t k = so[(size_t)i]; k < so[(size_t)i + 1]; k++) printf(" %d,%.17g,%.17g,%.17g,%d", ssid[(size_t)k], scov2[(size_t)k], sconf[(size_t)k], sabd[(size_t)k], sc1[(size_t)k]);
        printf("\n");
    }
    ald_tset_destroy(tm);
    return 0;
}
