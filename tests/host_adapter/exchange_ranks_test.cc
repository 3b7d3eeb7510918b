// exchange_ranks_test.cc -- GPU tier: the exchange by bucket owner with W ranks as THREADS of one process on one GPU, RCCL replaced by
// tests/host_adapter/mock_rccl.cc (ALD_RCCL_LIB).  Every rank decomposes its own shard of 200 graphs (one rank's shard is empty; ranks of
// equal parity draw the same graphs under other sample ids, so buckets are hit from several ranks), splits its finished transcripts by
// owner on the device (ald_batch_device_transcript_streams_by_owner), exchanges them all to all (ald_comm_exchange_streams), folds the
// segments it received in rank order into its own resident set (aletsch::owner_exchange_fold) and hands the set to ald_comm_gather_sets.
//   * rank 0's flat == the export of a host ald_tset fed all shards' UNSPLIT streams in rank order, array for array, bit for bit
//   * the per-rank item counts sum to the total, every item of rank r has hash % W == r
//   * mode "fail" (with ALD_MOCK_RCCL_FAIL_SEND=1): every rank gets an error from the exchange and is out of group mode afterwards
//   * mode "foreign": rank 1 folds its whole unsplit stream as well; ald_comm_gather_sets returns ALD_ERR_INVALID on ALL ranks
//   usage: exchange_ranks_test <world> [fail|foreign]
#include "../../aletsch_amd/host/owner_exchange.hpp"
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

enum { SHARD = 200 };
static const int64_t TID_BASE = (int64_t)3 << 44;

struct Arrays { int64_t n = 0; std::vector<uint64_t> hash; std::vector<unsigned char> bytes; };
template<class SizeFn, class ExportFn> static int export_arrays(SizeFn size, ExportFn exp, Arrays &A)
{
    int64_t n = 0, ne = 0, ns = 0;
    if(size(&n, &ne, &ns) != ALD_OK) return 1;
    std::vector<uint64_t> hash((size_t)n + 1); std::vector<int32_t> count((size_t)n + 1), count1((size_t)n + 1), count2((size_t)n + 1), lr(2 * (size_t)ne + 2), ssid((size_t)ns + 1), sc1((size_t)ns + 1);
    std::vector<char> strand((size_t)n + 1); std::vector<double> cov((size_t)n + 1), cov2((size_t)n + 1), conf((size_t)n + 1), abd((size_t)n + 1), scov2((size_t)ns + 1), sconf((size_t)ns + 1), sabd((size_t)ns + 1);
    std::vector<int64_t> tid((size_t)n + 1), eoff((size_t)n + 2), soff((size_t)n + 2);
    if(exp(hash.data(), count.data(), strand.data(), cov.data(), cov2.data(), conf.data(), abd.data(), count1.data(), count2.data(), tid.data(), eoff.data(), lr.data(),
           soff.data(), ssid.data(), scov2.data(), sconf.data(), sabd.data(), sc1.data()) != ALD_OK) return 1;
    A.n = n; A.hash.assign(hash.begin(), hash.begin() + n); A.bytes.clear();
    auto add = [&](const void *p, size_t bytes) { const unsigned char *c = (const unsigned char*)p; A.bytes.insert(A.bytes.end(), c, c + bytes); };
    add(hash.data(), 8 * (size_t)n); add(count.data(), 4 * (size_t)n); add(strand.data(), (size_t)n); add(cov.data(), 8 * (size_t)n); add(cov2.data(), 8 * (size_t)n); add(conf.data(), 8 * (size_t)n);
    add(abd.data(), 8 * (size_t)n); add(count1.data(), 4 * (size_t)n); add(count2.data(), 4 * (size_t)n); add(tid.data(), 8 * (size_t)n); add(eoff.data(), 8 * ((size_t)n + 1)); add(lr.data(), 8 * (size_t)ne);
    add(soff.data(), 8 * ((size_t)n + 1)); add(ssid.data(), 4 * (size_t)ns); add(scov2.data(), 8 * (size_t)ns); add(sconf.data(), 8 * (size_t)ns); add(sabd.data(), 8 * (size_t)ns); add(sc1.data(), 4 * (size_t)ns);
    return 0;
}
static int flat_arrays(const ald_tset_flat *f, Arrays &A)
{
    return export_arrays([&](int64_t *a, int64_t *b, int64_t *c) { return ald_tset_flat_size(f, a, b, c); },
                         [&](uint64_t *h, int32_t *c, char *s, double *v, double *v2, double *cf, double *ab, int32_t *c1, int32_t *c2, int64_t *t, int64_t *eo, int32_t *lr, int64_t *so, int32_t *ss, double *sv, double *sc, double *sa, int32_t *s1) {
                             return ald_tset_flat_export(f, h, c, s, v, v2, cf, ab, c1, c2, t, eo, lr, so, ss, sv, sc, sa, s1); }, A);
}

// graphs of rank r's shard into the batch: ranks of equal parity draw the same graphs
static int add_shard(ald_batch *b, int r, int n_graphs)
{
    ald_synth_spec sp; memset(&sp, 0, sizeof sp);
    sp.seed = 7100 + (uint64_t)(r % 2); sp.n_graphs = n_graphs; sp.v_min = 6; sp.v_max = 40; sp.edges_per_vertex = 3; sp.weight_mode = 2; sp.n_samples = 1; sp.phasing_per_graph = 2; sp.strand_mode = 1; sp.layout_mode = 1;
    int64_t tv = 0, te = 0, ts = 0, tp = 0, tpv = 0;
    if(ald_synth_sizes(&sp, &tv, &te, &ts, &tp, &tpv) != ALD_OK) return 1;
    const size_t n = (size_t)n_graphs;
    std::vector<int32_t> g_nv(n), g_ne(n), g_np(n), voff((size_t)tv + n), etgt((size_t)te + 1), esoff((size_t)te + n), sid((size_t)ts + 1), vl((size_t)tv + 1), vr((size_t)tv + 1), vt((size_t)tv + 1), poff((size_t)tp + n), pv((size_t)tpv + 1), pc((size_t)tp + 1);
    std::vector<double> ew((size_t)te + 1), eabd((size_t)te + 1), sabd((size_t)ts + 1), vw((size_t)tv + 1); std::vector<uint8_t> estr((size_t)te + 1); std::vector<char> gstr(n + 1);
    if(ald_synth_fill(&sp, g_nv.data(), g_ne.data(), g_np.data(), voff.data(), etgt.data(), ew.data(), estr.data(), eabd.data(), esoff.data(), sid.data(), sabd.data(), vw.data(), vl.data(), vr.data(), vt.data(),
                      poff.data(), pv.data(), pc.data(), gstr.data()) != ALD_OK) return 1;
    return ald_batch_add_packed(b, n_graphs, g_nv.data(), g_ne.data(), g_np.data(), voff.data(), etgt.data(), ew.data(), estr.data(), eabd.data(), esoff.data(), sid.data(), sabd.data(), vw.data(), vl.data(), vr.data(), vt.data(),
                                poff.data(), pv.data(), pc.data(), gstr.data(), nullptr, nullptr) != ALD_OK;
}

int main(int argc, char **argv)
{
    const int W = argc > 1 ? atoi(argv[1]) : 2; const std::string mode = argc > 2 ? argv[2] : "";
    const int empty_rank = W == 2 ? 0 : 2;                 // (never rank 1: the injected failure and the foreign bucket need rank 1 to have transcripts)
    uint8_t id[128];
    if(ald_comm_unique_id(id) != ALD_OK) { fprintf(stderr, "unique id: %s\n", ald_last_error()); return 2; }
    std::vector<int> rc(W, 0), gather_rc(W, 0); std::vector<std::vector<uint32_t>> unsplit((size_t)W); std::vector<Arrays> mine((size_t)W); Arrays merged;
    std::vector<std::thread> th;
    for(int r = 0; r < W; r++) th.emplace_back([&, r]() {
        auto fail = [&](int code, const char *what) { fprintf(stderr, "rank %d %s: %s\n", r, what, ald_last_error()); rc[r] = code; };
        ald_comm *c = nullptr; ald_batch *b = nullptr; ald_tset_dev *set = nullptr;
        if(ald_comm_create(id, W, r, 0, &c) != ALD_OK) return fail(3, "comm create");
        if(ald_batch_create(nullptr, 0, &b) != ALD_OK || ald_tset_dev_create(0, 0.8, &set) != ALD_OK) return fail(4, "create");
        const int ng = r == empty_rank ? 0 : SHARD; const int32_t graph_offset = r * SHARD;
        std::vector<int32_t> sid((size_t)ng + 1); for(int g = 0; g < ng; g++) sid[(size_t)g] = (g + r) % 5 - 1;
        do {
            // a rank without graphs runs no batch and passes W empty sub-streams
            if(ng) {
                if(add_shard(b, r, ng) || ald_batch_upload(b) != ALD_OK || ald_batch_run(b) != ALD_OK || ald_batch_download(b) != ALD_OK) { fail(5, "decompose"); break; }
                const uint32_t *w = nullptr; int64_t n = 0;
                if(ald_batch_transcript_stream(b, sid.data(), 0, &w, &n) != ALD_OK) { fail(5, "stream"); break; }
                unsplit[(size_t)r].assign(w, w + n);
            }
            const int e = aletsch::owner_exchange_fold(c, W, ng ? b : nullptr, ng ? sid.data() : nullptr, 0, graph_offset, set, TID_BASE);
            if(mode == "fail") {
                void *h = dlopen(getenv("ALD_RCCL_LIB"), RTLD_NOW | RTLD_NOLOAD);
                int (*in_group)() = h ? (int (*)())dlsym(h, "mock_rccl_thread_in_group") : nullptr;
                if(e == ALD_OK || !in_group || in_group() != 0) { fprintf(stderr, "rank %d: failed send not handled (rc=%d, in_group=%d)\n", r, e, in_group ? in_group() : -1); rc[r] = 6; }
                break;
            }
            if(e != ALD_OK) { fail(7, "exchange + fold"); break; }
            if(mode == "foreign" && r == 1 && ald_tset_dev_add_stream(set, unsplit[1].data(), (int64_t)unsplit[1].size(), nullptr, nullptr, graph_offset, TID_BASE, 0) != ALD_OK) { fail(8, "foreign add"); break; }
            ald_tset_flat *snap = nullptr, *all = nullptr;
            if(ald_tset_dev_snapshot(set, &snap) != ALD_OK) { fail(9, "snapshot"); break; }
            gather_rc[r] = ald_comm_gather_sets(c, snap, &all);
            if(mode == "foreign") { if(gather_rc[r] != ALD_ERR_INVALID || all) { fprintf(stderr, "rank %d: foreign bucket not refused (rc=%d)\n", r, gather_rc[r]); rc[r] = 10; } ald_tset_flat_free(snap); break; }
            if(gather_rc[r] != ALD_OK) { fail(11, "gather sets"); ald_tset_flat_free(snap); break; }
            if(flat_arrays(snap, mine[(size_t)r])) rc[r] = 12;
            if((r == 0) != (all != nullptr)) rc[r] = 13;
            if(all && flat_arrays(all, merged)) rc[r] = 12;
            ald_tset_flat_free(snap); ald_tset_flat_free(all);
        } while(0);
        ald_tset_dev_destroy(set); ald_batch_destroy(b); ald_comm_destroy(c);
    });
    for(auto &t : th) t.join();
    int bad = 0; for(int r = 0; r < W; r++) if(rc[r]) { fprintf(stderr, "rank %d: failure code %d\n", r, rc[r]); bad = 1; }
    if(bad) return 1;
    if(mode == "fail") { printf("EXCHANGE_RANKS_OK world=%d (injected send failure handled on every rank)\n", W); return 0; }
    if(mode == "foreign") { printf("EXCHANGE_RANKS_OK world=%d (foreign bucket refused on every rank)\n", W); return 0; }
    // the yardstick: a host set fed all shards' unsplit streams in rank order
    ald_tset *host = nullptr;
    if(ald_tset_create(0.8, &host) != ALD_OK) return 2;
    for(int r = 0; r < W; r++) if(ald_tset_add_stream(host, unsplit[(size_t)r].data(), (int64_t)unsplit[(size_t)r].size(), r * SHARD, TID_BASE) != ALD_OK) { fprintf(stderr, "host add: %s\n", ald_last_error()); return 2; }
    Arrays want;
    if(export_arrays([&](int64_t *a, int64_t *b, int64_t *c) { return ald_tset_size(host, a, b, c); },
                     [&](uint64_t *h, int32_t *c, char *s, double *v, double *v2, double *cf, double *ab, int32_t *c1, int32_t *c2, int64_t *t, int64_t *eo, int32_t *lr, int64_t *so, int32_t *ss, double *sv, double *sc, double *sa, int32_t *s1) {
                         return ald_tset_export(host, h, c, s, v, v2, cf, ab, c1, c2, t, eo, lr, so, ss, sv, sc, sa, s1); }, want)) return 2;
    ald_tset_destroy(host);
    int64_t sum = 0, most = 0;
    for(int r = 0; r < W; r++) {
        sum += mine[(size_t)r].n; if(mine[(size_t)r].n > most) most = mine[(size_t)r].n;
        for(uint64_t h : mine[(size_t)r].hash) if((int)(h % (uint64_t)W) != r) { fprintf(stderr, "rank %d holds bucket %llu\n", r, (unsigned long long)h); return 3; }
    }
    if(sum != want.n || merged.n != want.n) { fprintf(stderr, "item counts: ranks %lld, merged %lld, host %lld\n", (long long)sum, (long long)merged.n, (long long)want.n); return 3; }
    if(merged.bytes != want.bytes) { fprintf(stderr, "rank 0's merged set differs from the host set (%lld items)\n", (long long)want.n); return 3; }
    if(want.n < 500) { fprintf(stderr, "only %lld items: the shards are too small to show anything\n", (long long)want.n); return 3; }
    printf("EXCHANGE_RANKS_OK world=%d items=%lld largest_share=%.3f\n", W, (long long)want.n, (double)most / (double)want.n);
    return 0;
}
