// finish_test.cc -- gpu_scallop_batch::flush_on_device (aletsch_amd/host/gpu_scallop.hpp): enqueue -> flush_on_device() ->
// ald_tset_dev_add_batch(handle()) gives the items of the flush() path, and status(i) answers after either flush.  Round 0 ends the run
// with flush() (upload, run, download), round 1 with flush_on_device() (upload, run, finish: no record leaves the device); each round folds
// its batch into a device set of its own; the exported arrays of the two sets are compared byte for byte.
// Reads N graphs from stdin in adapter_test's format ("V E P", V lines "w lpos rpos", E lines "s t w", P lines "len count v...").
// Prints "items <n> host_items <h> equal" and exits 0; exit status 3 when the sets or the status words differ.
// Driven by tests/test_finish_gpu.py; tests/test_finish_cpu.py checks that it compiles as C++11 without a warning.
#include "../../aletsch_amd/host/gpu_scallop.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <unordered_map>

struct mock_edge { int s, t; int source() const { return s; } int target() const { return t; } };
struct mock_edge_info { int strand = 0, count = 0; double abd = 0; std::set<int> samples; std::unordered_map<int, double> spAbd; };
struct mock_vertex_info { int32_t lpos = 0, rpos = 0; int type = -1; };
struct mock_graph {
    std::vector<mock_edge*> es; std::vector<double> ew; std::vector<mock_edge_info> ei; std::vector<double> vw; std::vector<mock_vertex_info> vi; char strand = '.';
    size_t num_vertices() const { return vw.size(); }
    std::pair<std::vector<mock_edge*>::iterator, std::vector<mock_edge*>::iterator> edges() { return {es.begin(), es.end()}; }
    int idx(mock_edge *e) const { for(size_t i = 0; i < es.size(); i++) if(es[i] == e) return (int)i; return -1; }
    double get_edge_weight(mock_edge *e) const { return ew[idx(e)]; }
    const mock_edge_info &get_edge_info(mock_edge *e) const { return ei[idx(e)]; }
    double get_vertex_weight(int v) const { return vw[v]; }
    const mock_vertex_info &get_vertex_info(int v) const { return vi[v]; }
};
struct mock_hyper_set { std::map<std::vector<int>, int> nodes; };
struct mock_parameters { double max_decompose_error_ratio[8] = {0.30, 0.00, 1.10, 1.10, 0.75, 0.30, 0.00, 1.00}; double min_guaranteed_edge_weight = 0.01, min_transcript_coverage = 2.0; int max_num_exons = 10000; };
struct mock_path { std::vector<int> v; std::vector<std::pair<int, int>> junc; int length = 0; double abd = 0, weight = 0, conf = 0, reads = 0; char strand = '.'; int count = 0; };

static bool read_graph(mock_graph &g, mock_hyper_set &hs)
{
    int V, E, P;
    if(scanf("%d %d %d", &V, &E, &P) != 3) return false;
    for(int i = 0; i < V; i++) { double w; int l, r; if(scanf("%lf %d %d", &w, &l, &r) != 3) return false; g.vw.push_back(w); mock_vertex_info vi; vi.lpos = l; vi.rpos = r; g.vi.push_back(vi); }
    for(int k = 0; k < E; k++) { int s, t; double w; if(scanf("%d %d %lf", &s, &t, &w) != 3) return false; g.es.push_back(new mock_edge{s, t}); g.ew.push_back(w); mock_edge_info ei; ei.count = 1; ei.abd = w; ei.samples.insert(0); ei.spAbd[0] = w; g.ei.push_back(ei); }
    for(int p = 0; p < P; p++) { int len, c; if(scanf("%d %d", &len, &c) != 2) return false; std::vector<int> v((size_t)len); for(int &x : v) if(scanf("%d", &x) != 1) return false; hs.nodes[v] += c; }
    return true;
}

// every array ald_tset_dev_export fills, back to back, as bytes
static int export_bytes(const ald_tset_dev *s, std::vector<unsigned char> &out, long long &n_items, long long &n_host)
{
    int64_t n = 0, ne = 0, ns = 0, dev = 0, host = 0;
    if(ald_tset_dev_size(s, &n, &ne, &ns) != ALD_OK || ald_tset_dev_stats(s, nullptr, nullptr, &dev, &host) != ALD_OK) return 1;
    std::vector<uint64_t> hash((size_t)n + 1); std::vector<int32_t> count((size_t)n + 1), count1((size_t)n + 1), count2((size_t)n + 1), lr(2 * (size_t)ne + 2), ssid((size_t)ns + 1), sc1((size_t)ns + 1);
    std::vector<char> strand((size_t)n + 1); std::vector<double> cov((size_t)n + 1), cov2((size_t)n + 1), conf((size_t)n + 1), abd((size_t)n + 1), scov2((size_t)ns + 1), sconf((size_t)ns + 1), sabd((size_t)ns + 1);
    std::vector<int64_t> tid((size_t)n + 1), eoff((size_t)n + 2), soff((size_t)n + 2);
    if(ald_tset_dev_export(s, hash.data(), count.data(), strand.data(), cov.data(), cov2.data(), conf.data(), abd.data(), count1.data(), count2.data(), tid.data(), eoff.data(), lr.data(),
                           soff.data(), ssid.data(), scov2.data(), sconf.data(), sabd.data(), sc1.data()) != ALD_OK) return 1;
    out.clear();
    auto add = [&](const void *p, size_t bytes) { const unsigned char *c = (const unsigned char*)p; out.insert(out.end(), c, c + bytes); };
    add(hash.data(), 8 * (size_t)n); add(count.data(), 4 * (size_t)n); add(strand.data(), (size_t)n); add(cov.data(), 8 * (size_t)n); add(cov2.data(), 8 * (size_t)n); add(conf.data(), 8 * (size_t)n);
    add(abd.data(), 8 * (size_t)n); add(count1.data(), 4 * (size_t)n); add(count2.data(), 4 * (size_t)n); add(tid.data(), 8 * (size_t)n); add(eoff.data(), 8 * ((size_t)n + 1)); add(lr.data(), 8 * (size_t)ne);
    add(soff.data(), 8 * ((size_t)n + 1)); add(ssid.data(), 4 * (size_t)ns); add(scov2.data(), 8 * (size_t)ns); add(sconf.data(), 8 * (size_t)ns); add(sabd.data(), 8 * (size_t)ns); add(sc1.data(), 4 * (size_t)ns);
    n_items = (long long)n; n_host = (long long)host;
    return 0;
}

int main()
{
    mock_parameters cfg;
    int N;
    if(scanf("%d", &N) != 1) return 2;
    std::vector<mock_graph> gs((size_t)N); std::vector<mock_hyper_set> hs((size_t)N);
    for(int n = 0; n < N; n++) if(!read_graph(gs[(size_t)n], hs[(size_t)n])) return 2;
    std::vector<int32_t> sid((size_t)N); for(int n = 0; n < N; n++) sid[(size_t)n] = n % 5 - 1;
    std::vector<unsigned char> bytes[2]; std::vector<int> status[2]; long long items[2] = {0, 0}, host[2] = {0, 0};
    try {
        aletsch::gpu_scallop_batch<mock_graph, mock_hyper_set, mock_parameters, mock_path> batch(cfg, 0);
        for(int round = 0; round < 2; round++) {
            ald_tset_dev *set = nullptr;
            if(ald_tset_dev_create(0, 0.8, &set) != ALD_OK) return 2;
            std::vector<int> t;
            for(int n = 0; n < N; n++) t.push_back(batch.enqueue(gs[(size_t)n], hs[(size_t)n]));
            if(round == 0) batch.flush(); else batch.flush_on_device();
            for(int n = 0; n < N; n++) status[round].push_back(batch.status(t[(size_t)n]));
            const int rc = ald_tset_dev_add_batch(set, batch.handle(), sid.data(), 0, 0);
            if(rc != ALD_OK) { fprintf(stderr, "ald_tset_dev_add_batch: %d %s\n", rc, ald_last_error()); ald_tset_dev_destroy(set); return 1; }
            const int bad = export_bytes(set, bytes[round], items[round], host[round]);
            ald_tset_dev_destroy(set);
            if(bad) return 2;
            batch.clear();
        }
    } catch(const std::exception &e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    if(status[0] != status[1]) { fprintf(stderr, "status words differ between flush() and flush_on_device()\n"); return 3; }
    if(items[0] != items[1] || host[0] != host[1] || bytes[0] != bytes[1]) { fprintf(stderr, "the sets differ: %lld / %lld items\n", items[0], items[1]); return 3; }
    printf("items %lld host_items %lld equal\n", items[1], host[1]);
    return 0;
}
