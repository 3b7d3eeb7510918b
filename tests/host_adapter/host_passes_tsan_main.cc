// host_passes_tsan_main.cc -- TEST-ONLY: the host passes that go multi-threaded only above a size threshold (host_pack.h: the check-and-copy
// pass of add_packed, the raw-graph verdict pass, the byte-sliced copy of pack_range, HostResults::build; ald_sink.cpp: the transcript
// stream and the merges), each made ABOVE its threshold in a CPU program built with -fsanitize=thread, and compared word for word with
// the same call made with one thread, one after the other in this program.  Driven by tests/test_host_threads_cpu.py.
//
// The thresholds are not restated here: the graph set is simply large (argv[1] graphs, default 12000, of 6..16 vertices), every case
// asks for 4 threads (16 for the sink as well) and reads from tests/host_adapter/thread_probe.h how many the call really started; a case
// whose pass ran narrower than asked FAILS.  Every case prints the widths it ran with.
//
// HostResults::build takes its pool from ONE emulation run of the graph set (the run the sink cases need anyway, so the cheaper choice;
// the emulation's class objects are not instrumented): the index it is given again is the decoded table of that run.
// ald_tset_merge is not here: it is a serial loop over the shards (ald_sink.cpp), no thread is started in it.
#include "../../aletsch_amd/csrc/ald_internal.h"
#include "stub_control.h"
#include <random>

namespace {

int failures = 0;
void check(bool ok, const char *what) { if(!ok) { failures++; printf("FAILED %s\n", what); } }

// n canonical graphs back to back in the layout of ald_batch_add_packed; graph i is RAW (phases instead of phasing lists) when i % 7 == 3
struct packed {
    std::vector<int32_t> nv, ne, np, voff, etgt, esoff, sid, lpos, rpos, vtype, poff, pv, pc, ecount, raw_dist, nph, rpoff, rpcoord, rpcount;
    std::vector<double> ew, eabd, sabd, vw; std::vector<uint8_t> estrand; std::vector<char> gstrand;
    std::vector<int64_t> e_at, vo_at;          // first edge / first vertex_offset entry of every graph
    int n() const { return (int)nv.size(); }
};
packed make_graphs(int n, unsigned seed)
{
    packed P; std::mt19937 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    for(int g = 0; g < n; g++) {
        const int V = rnd(6, 16); const bool raw = g % 7 == 3;
        std::vector<std::vector<int>> row((size_t)V);
        for(int s = 0; s + 1 < V; s++) {
            row[(size_t)s].push_back(s + 1);                                     // a chain: every inner vertex has an edge in and one out
            for(int t = s + 2; t < V; t++) if(!(s == 0 && t == V - 1) && rng() % 5 == 0) row[(size_t)s].push_back(t);
        }
        P.e_at.push_back((int64_t)P.etgt.size()); P.vo_at.push_back((int64_t)P.voff.size());
        int E = 0; P.voff.push_back(0); P.esoff.push_back(0);
        for(int s = 0; s < V; s++) {
            for(int t : row[(size_t)s]) {
                const double w = 1.0 + (double)(rng() % 4000) / 16.0;
                P.etgt.push_back(t); P.ew.push_back(w); P.eabd.push_back(w); P.estrand.push_back(0); P.ecount.push_back(1);
                P.sid.push_back(0); P.sabd.push_back(w); E++; P.esoff.push_back(E);
            }
            P.voff.push_back(E);
        }
        int pos = 1000;
        for(int v = 0; v < V; v++) {
            const int len = (v == 0 || v == V - 1) ? 0 : rnd(30, 300);
            P.vw.push_back(1.0 + (double)(rng() % 1000) / 8.0); P.lpos.push_back(pos); P.rpos.push_back(pos + len); P.vtype.push_back(-1);
            pos += len + (rng() % 3 == 0 ? 0 : rnd(50, 900));                    // some exons touch their successor
        }
        const size_t v0 = P.lpos.size() - (size_t)V;
        P.nv.push_back(V); P.ne.push_back(E); P.gstrand.push_back("+-."[g % 3]);
        P.poff.push_back(0); P.rpoff.push_back(0);
        if(raw) {            // one phase over the first two inner exons, in coordinates
            P.np.push_back(0); P.raw_dist.push_back(10000); P.nph.push_back(1);
            for(int v = 1; v <= 2; v++) { P.rpcoord.push_back(P.lpos[v0 + (size_t)v]); P.rpcoord.push_back(P.rpos[v0 + (size_t)v]); }
            P.rpoff.push_back(4); P.rpcount.push_back(rnd(1, 9));
        } else {             // two phasing lists, ascending and in lexicographic order
            P.np.push_back(2); P.raw_dist.push_back(-1); P.nph.push_back(0);
            P.pv.push_back(1); P.pv.push_back(2); P.poff.push_back(2); P.pc.push_back(rnd(1, 9));
            P.pv.push_back(2); P.pv.push_back(3); P.pv.push_back(4); P.poff.push_back(5); P.pc.push_back(rnd(1, 9));
        }
    }
    return P;
}
int add_plain(HostBatch &B, const packed &P)
{
    return B.add_packed(P.n(), P.nv.data(), P.ne.data(), P.np.data(), P.voff.data(), P.etgt.data(), P.ew.data(), P.estrand.data(), P.eabd.data(), P.esoff.data(), P.sid.data(), P.sabd.data(),
                        P.vw.data(), P.lpos.data(), P.rpos.data(), P.vtype.data(), P.poff.data(), P.pv.data(), P.pc.data(), P.gstrand.data(), P.ecount.data(), nullptr);
}
int add_raw(HostBatch &B, const packed &P)
{
    return B.add_packed_raw(P.n(), P.nv.data(), P.ne.data(), P.np.data(), P.voff.data(), P.etgt.data(), P.ew.data(), P.estrand.data(), P.eabd.data(), P.esoff.data(), P.sid.data(), P.sabd.data(),
                            P.vw.data(), P.lpos.data(), P.rpos.data(), P.vtype.data(), P.poff.data(), P.pv.data(), P.pc.data(), P.gstrand.data(), P.ecount.data(), nullptr,
                            P.raw_dist.data(), P.nph.data(), P.rpoff.data(), P.rpcoord.data(), P.rpcount.data());
}
// every graph staged: the raw marks dropped (those graphs then simply have no phasing lists)
packed without_raw(packed P) { std::fill(P.raw_dist.begin(), P.raw_dist.end(), -1); return P; }

template<class V> bool same_vec(const V &a, const V &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); }
bool same_batch(const HostBatch &a, const HostBatch &b)
{
#define ALD_SAME(f) same_vec(a.f, b.f)
    return ALD_SAME(g_nv) && ALD_SAME(g_ne) && ALD_SAME(g_np) && ALD_SAME(off_v) && ALD_SAME(off_e) && ALD_SAME(off_s) && ALD_SAME(off_p) && ALD_SAME(off_pv) && ALD_SAME(vertex_offset) && ALD_SAME(edge_target)
        && ALD_SAME(edge_weight) && ALD_SAME(edge_strand) && ALD_SAME(edge_abd) && ALD_SAME(edge_sample_offset) && ALD_SAME(sample_id) && ALD_SAME(sample_abd) && ALD_SAME(vertex_weight) && ALD_SAME(vertex_lpos)
        && ALD_SAME(vertex_rpos) && ALD_SAME(vertex_type) && ALD_SAME(in_offset) && ALD_SAME(in_edge) && ALD_SAME(phasing_offset) && ALD_SAME(phasing_vertex) && ALD_SAME(phasing_count) && ALD_SAME(graph_strand)
        && ALD_SAME(edge_count) && ALD_SAME(edge_rank) && ALD_SAME(g_rawdist) && ALD_SAME(off_rp) && ALD_SAME(off_rc) && ALD_SAME(rphase_offset) && ALD_SAME(rphase_coord) && ALD_SAME(rphase_count) && ALD_SAME(g_sid)
        && a.has_rank == b.has_rank && a.has_raw == b.has_raw && a.def_eabd == b.def_eabd && a.def_ecount == b.def_ecount && a.def_vtype == b.def_vtype && a.def_estrand == b.def_estrand && a.uni_samples == b.uni_samples && a.err == b.err;
#undef ALD_SAME
}
void threads(const char *var, int k) { setenv(var, std::to_string(k).c_str(), 1); }      // (only ever called while no other thread runs)

// one staging call with 1 and with 4 threads, each into a batch that already holds `head`; rc and batch must agree, the threaded call
// must have started at least `min_started` threads (3 per pass that is to run 4 wide)
void staging_case(const char *name, const packed &head, const packed &P, bool raw, int want_rc, long min_started)
{
    HostBatch B[2]; int rc[2]; long started = 0, peak = 0;
    for(int k = 0; k < 2; k++) {
        threads("ALD_STAGE_THREADS", k ? 4 : 1);
        check(add_plain(B[k], head) == ALD_OK, "staging the head of the batch");
        thread_probe_reset();
        rc[k] = raw ? add_raw(B[k], P) : add_plain(B[k], P);
        if(k) { started = thread_probe().started; peak = thread_probe().peak; } else check(thread_probe().started == 0, "the one-thread call started a thread");
    }
    check(rc[0] == want_rc && rc[1] == want_rc, "return code"); check(same_batch(B[0], B[1]), "the batch differs between 1 and 4 threads");
    check(peak + 1 >= 4 && started >= min_started, "a staging pass ran narrower than 4 threads");
    check(B[0].n() == head.n() + (want_rc == ALD_OK ? P.n() : 0), "graphs in the batch (all or nothing)");
    printf("CASE %s staging=%ld started=%ld graphs=%d edges=%lld rc=%d %s\n", name, peak + 1, started, P.n(), (long long)P.etgt.size(), rc[1], failures ? "FAILED" : "OK");
}

struct flat_set {
    int64_t n = 0, ne = 0, ns = 0; std::vector<uint8_t> bytes;
    bool fetch(const ald_tset *t)
    {
        if(ald_tset_size(t, &n, &ne, &ns) != ALD_OK) return false;
        const size_t N = (size_t)n, NE = (size_t)ne, NS = (size_t)ns;
        std::vector<uint64_t> h(N + 1); std::vector<int32_t> cnt(N + 1), c1(N + 1), c2(N + 1), lr(2 * NE + 2), ssid(NS + 1), sc1(NS + 1); std::vector<char> st(N + 1);
        std::vector<double> cov(N + 1), cov2(N + 1), conf(N + 1), abd(N + 1), scov2(NS + 1), sconf(NS + 1), sabd(NS + 1); std::vector<int64_t> tid(N + 1), eo(N + 2), so(N + 2);
        if(ald_tset_export(t, h.data(), cnt.data(), st.data(), cov.data(), cov2.data(), conf.data(), abd.data(), c1.data(), c2.data(), tid.data(), eo.data(), lr.data(),
                           so.data(), ssid.data(), scov2.data(), sconf.data(), sabd.data(), sc1.data()) != ALD_OK) return false;
        bytes.clear();
        auto put = [&](const void *p, size_t k) { bytes.insert(bytes.end(), (const uint8_t*)p, (const uint8_t*)p + k); };
        put(h.data(), 8 * N); put(cnt.data(), 4 * N); put(st.data(), N); put(cov.data(), 8 * N); put(cov2.data(), 8 * N); put(conf.data(), 8 * N); put(abd.data(), 8 * N); put(c1.data(), 4 * N); put(c2.data(), 4 * N);
        put(tid.data(), 8 * N); put(eo.data(), 8 * (N + 1)); put(lr.data(), 8 * NE); put(so.data(), 8 * (N + 1)); put(ssid.data(), 4 * NS); put(scov2.data(), 8 * NS); put(sconf.data(), 8 * NS); put(sabd.data(), 8 * NS); put(sc1.data(), 4 * NS);
        return true;
    }
    bool operator==(const flat_set &o) const { return n == o.n && ne == o.ne && ns == o.ns && bytes == o.bytes; }
};

} // namespace

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 12000;
    stub_reset();
    const packed all = make_graphs(n, 20261020u), head = without_raw(make_graphs(100, 7u));
    const packed plain = without_raw(all);

    // ---- add_packed / add_packed_raw: clean, then with a defect in the middle of the call ----
    staging_case("add_packed", head, plain, false, ALD_OK, 3);
    staging_case("add_packed_raw", head, all, true, ALD_OK, 6);
    {   // a row whose targets are not in ascending order: the threaded pass gives its verdict, the batch is rolled back, the per-graph path sorts
        packed bad = plain; int g = n / 2; while(bad.voff[(size_t)bad.vo_at[(size_t)g] + 1] < 2) g++;
        const size_t e = (size_t)bad.e_at[(size_t)g]; std::swap(bad.etgt[e], bad.etgt[e + 1]); std::swap(bad.ew[e], bad.ew[e + 1]); std::swap(bad.eabd[e], bad.eabd[e + 1]); std::swap(bad.sabd[e], bad.sabd[e + 1]);
        staging_case("add_packed_noncanonical_row", head, bad, false, ALD_OK, 3);
        HostBatch A, B; threads("ALD_STAGE_THREADS", 4); add_plain(A, bad); add_plain(B, plain);
        check(same_vec(A.edge_target, B.edge_target) && same_vec(A.edge_weight, B.edge_weight), "the per-graph path did not put the row in order");
    }
    {   // a raw graph with parallel edges out of the source: refused by the verdict pass, the whole call taken back
        packed bad = all; int g = n / 2; while(bad.raw_dist[(size_t)g] < 0 || bad.voff[(size_t)bad.vo_at[(size_t)g] + 1] < 2) g++;
        const size_t e = (size_t)bad.e_at[(size_t)g]; bad.etgt[e + 1] = bad.etgt[e];
        staging_case("add_packed_raw_parallel_source_edges", head, bad, true, ALD_ERR_INVALID, 6);
    }

    // ---- pack_range: the wire buffer in byte slices ----
    HostBatch big; threads("ALD_STAGE_THREADS", 4); check(add_raw(big, all) == ALD_OK, "staging the whole set");
    {
        HostBatch::Section sec[HostBatch::S_COUNT]; const uint64_t bytes = big.layout(sec);
        std::vector<uint8_t> w1((size_t)bytes, 0), w4((size_t)bytes, 0);
        threads("ALD_STAGE_THREADS", 1); thread_probe_reset(); big.pack_into(w1.data(), sec); check(thread_probe().started == 0, "the one-thread copy started a thread");
        threads("ALD_STAGE_THREADS", 4); thread_probe_reset(); big.pack_into(w4.data(), sec);
        check(w1 == w4, "the wire buffer differs between 1 and 4 threads"); check(thread_probe().peak + 1 >= 4, "the byte-sliced copy ran narrower than 4 threads");
        printf("CASE pack_range staging=%ld bytes=%llu %s\n", thread_probe().peak + 1, (unsigned long long)bytes, failures ? "FAILED" : "OK");
    }

    // ---- one emulation run of the set through the stand-in: the downloaded batch every case below reads ----
    ald_params prm; { const double r[8] = {0.30, 0.00, 1.10, 1.10, 0.75, 0.30, 0.00, 1.00}; for(int i = 0; i < 8; i++) prm.max_decompose_error_ratio[i] = r[i]; prm.min_guaranteed_edge_weight = 0.01; prm.min_transcript_coverage = 2.0; prm.max_num_exons = 10000; prm.reserved = 0; }
    ald_batch *b = nullptr; check(ald_batch_create(&prm, 0, &b) == ALD_OK, "ald_batch_create");
    threads("ALD_STAGE_THREADS", 4);
    check(ald_batch_add_packed_raw(b, all.n(), all.nv.data(), all.ne.data(), all.np.data(), all.voff.data(), all.etgt.data(), all.ew.data(), all.estrand.data(), all.eabd.data(), all.esoff.data(), all.sid.data(), all.sabd.data(),
                                   all.vw.data(), all.lpos.data(), all.rpos.data(), all.vtype.data(), all.poff.data(), all.pv.data(), all.pc.data(), all.gstrand.data(), all.ecount.data(), nullptr,
                                   all.raw_dist.data(), all.nph.data(), all.rpoff.data(), all.rpcoord.data(), all.rpcount.data()) == ALD_OK, "ald_batch_add_packed_raw");
    check(ald_batch_upload(b) == ALD_OK && ald_batch_run(b) == ALD_OK && ald_batch_download(b) == ALD_OK, "the emulation run");
    if(failures) { printf("FAILED before the result cases: %s\n", ald_last_error()); return 1; }
    const HostResults &R = b->res; const int64_t np = R.n_paths();
    long ok_graphs = 0; for(int g = 0; g < n; g++) ok_graphs += R.status[(size_t)g] == ALD_ST_OK;

    // ---- HostResults::build: the same pool decoded again through the table of the run ----
    {
        std::vector<int32_t> npaths((size_t)n); std::vector<long long> first((size_t)n); std::vector<unsigned long long> index(R.rec_off.begin(), R.rec_off.end());
        for(int g = 0; g < n; g++) { npaths[(size_t)g] = (int32_t)(R.path_begin[(size_t)g + 1] - R.path_begin[(size_t)g]); first[(size_t)g] = (long long)R.path_begin[(size_t)g]; }
        HostResults H[2]; long peak = 0;
        for(int k = 0; k < 2; k++) {
            H[k].status = R.status; H[k].n_iters = R.n_iters; H[k].ext_pool = R.pool_data(); H[k].ext_words = R.pool_size();
            threads("ALD_STAGE_THREADS", k ? 4 : 1); thread_probe_reset();
            check(H[k].build(n, npaths.data(), index.data(), (uint64_t)index.size(), first.data()) == 0, "HostResults::build");
            if(k) peak = thread_probe().peak; else check(thread_probe().started == 0, "the one-thread decode started a thread");
        }
        for(int k = 0; k < 2; k++) check(same_vec(H[k].rec_off, R.rec_off) && same_vec(H[k].coverage, R.coverage) && same_vec(H[k].chain_key, R.chain_key) && same_vec(H[k].n_exon_words, R.n_exon_words)
                                         && H[k].path_begin == R.path_begin && H[k].attempt == R.attempt && H[k].out_bytes == R.out_bytes, "the decoded table differs");
        check(peak + 1 >= 4, "the decode ran narrower than 4 threads");
        printf("CASE results_build staging=%ld paths=%lld graphs_ok=%ld %s\n", peak + 1, (long long)np, ok_graphs, failures ? "FAILED" : "OK");
    }

    // ---- the sink: stream, add_stream, add_batch with 1, 4 and 16 threads, against one ald_tset_add per graph ----
    std::vector<int32_t> sid((size_t)n); for(int g = 0; g < n; g++) sid[(size_t)g] = g % 3;
    flat_set want;
    {
        ald_tset *ref = nullptr; check(ald_tset_create(0.8, &ref) == ALD_OK, "ald_tset_create");
        for(int g = 0; g < n; g++) {
            const int64_t a = R.path_begin[(size_t)g], c = R.path_begin[(size_t)g + 1] - a; if(!c) continue;
            std::vector<char> st; std::vector<double> cov, conf, abd; std::vector<int32_t> c1, lr; std::vector<int64_t> tid, eo(1, 0);
            for(int64_t k = 0; k < c; k++) {
                ald_transcript_view tv; check(ald_batch_get_transcript(b, g, (int32_t)k, &tv) == ALD_OK, "ald_batch_get_transcript");
                st.push_back(tv.strand); cov.push_back(tv.coverage); conf.push_back(tv.conf); abd.push_back(tv.abd); c1.push_back(tv.count1); tid.push_back(((int64_t)g << 20) | k);
                lr.insert(lr.end(), tv.exons, tv.exons + 2 * tv.num_exons); eo.push_back(eo.back() + tv.num_exons);
            }
            const int64_t grp[2] = {0, c}; lr.push_back(0);
            check(ald_tset_add(ref, 1, grp, &sid[(size_t)g], st.data(), cov.data(), conf.data(), abd.data(), c1.data(), tid.data(), eo.data(), lr.data(), 0) == ALD_OK, "ald_tset_add");
        }
        check(want.fetch(ref), "export of the per-graph loop"); ald_tset_destroy(ref);
    }
    std::vector<uint32_t> stream1;
    for(int k : {1, 4, 16}) {
        threads("ALD_SINK_THREADS", k);
        const uint32_t *words = nullptr; int64_t nw = 0;
        thread_probe_reset(); check(ald_batch_transcript_stream(b, sid.data(), 0, &words, &nw) == ALD_OK, "ald_batch_transcript_stream"); const long w_stream = thread_probe().peak + 1;
        std::vector<uint32_t> stream(words, words + nw); if(k == 1) stream1 = stream; check(stream == stream1, "the transcript stream differs from the one-thread stream");
        ald_tset *ts = nullptr, *tb = nullptr; check(ald_tset_create(0.8, &ts) == ALD_OK && ald_tset_create(0.8, &tb) == ALD_OK, "ald_tset_create");
        thread_probe_reset(); check(ald_tset_add_stream(ts, stream.data(), nw, 0, 0) == ALD_OK, "ald_tset_add_stream"); const long w_add = thread_probe().peak + 1;
        stub_reset(); check(ald_tset_add_batch(tb, b, sid.data(), 0, 0) == ALD_OK, "ald_tset_add_batch"); const long w_batch = stub_sink_width_min();
        flat_set fs, fb; check(fs.fetch(ts) && fb.fetch(tb), "export");
        check(fs == want, "ald_tset_add_stream differs from the per-graph loop"); check(fb == want, "ald_tset_add_batch differs from the per-graph loop");
        check(w_stream == k && w_add == k && w_batch == k, "a sink pass did not run as wide as asked");
        printf("CASE sink sink=%d stream=%ld add_stream=%ld add_batch=%ld transcripts=%lld items=%lld %s\n", k, w_stream, w_add, w_batch, (long long)np, (long long)want.n, failures ? "FAILED" : "OK");
        ald_tset_destroy(ts); ald_tset_destroy(tb);
    }
    ald_batch_destroy(b);
    printf(failures ? "HOST PASSES FAILED (%d)\n" : "HOST PASSES OK\n", failures);
    return failures ? 1 : 0;
}
