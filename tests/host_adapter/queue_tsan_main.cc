// queue_tsan_main.cc -- TEST-ONLY: aletsch::gpu_assembly_queue (aletsch_amd/host/gpu_dispatch.hpp) and, under it, the threaded merge of the
// result sink (aletsch_amd/csrc/ald_sink.cpp) in a CPU program built with -fsanitize=thread; the batch entry points are those of
// stub_batch_abi.cc (real staging, the engine's emulation as the device).  Driven by tests/test_host_threads_cpu.py.
//
//   queue_tsan_main T D P S                 clean run: T submitting threads, D device slots, P pack threads, S batch objects per device
//   queue_tsan_main T D P S ENTRY K         error run: the Kth call of ENTRY (stub_control.h) fails in the middle of the run
// stdin: "N R", then N graphs and R raw graphs in the text form of mock_types.h; every fifth item of the run is a raw graph while there
// are any left (submit_raw, so chunks with any_raw go through ald_batch_add_packed_raw), item i carries sample id i % 3.
// batch_graphs = 64 and chunk_graphs = 8: dozens of batches, every slot reused several times, submitters held back by the ready cap.
//
// A clean run makes three rounds: (1) T threads submit the first third to queue A, drain; (2) T OTHER threads submit the second third
// to queue A (new lanes, partial chunks, reused slots), drain; queue A is destroyed and queue B constructed; (3) the threads of round 1,
// which have outlived queue A and still hold its lane in thread-local storage, submit the rest to queue B, drain.  The sink is then
// compared with a serial loop -- one ald_tset_add per graph in ticket order over ONE emulation run of all graphs: exactly equal with one
// submitter, and as tests/test_gpu_adapter.py::test_dispatch_queue_matches_the_serial_merge compares for several.
#include "mock_types.h"
#include "stub_control.h"
#include <cmath>
#include <cstring>
#include <string>

typedef aletsch::gpu_assembly_queue<mock_graph, mock_hyper_set, mock_parameters> queue_t;

struct item { mock_graph *g; mock_hyper_set *hs; mock_phase_set px; bool raw; int sid; };
static std::vector<item> items;

static void submit_item(queue_t &q, size_t i)
{
    item &it = items[i];
    if(it.raw) q.submit_raw(*it.g, it.px, it.sid); else q.submit(*it.g, *it.hs, it.sid);
}

// the exported set, every column
struct flat_set {
    int64_t n = 0, ne = 0, ns = 0;
    std::vector<uint64_t> h; std::vector<int32_t> cnt, c1, c2, lr, ssid, sc1; std::vector<char> st; std::vector<double> cov, cov2, conf, abd, scov2, sconf, sabd; std::vector<int64_t> tid, eo, so;
    bool fetch(const ald_tset *t)
    {
        if(ald_tset_size(t, &n, &ne, &ns) != ALD_OK) return false;
        h.resize((size_t)n + 1); cnt.resize((size_t)n + 1); c1.resize((size_t)n + 1); c2.resize((size_t)n + 1); lr.resize(2 * (size_t)ne + 2); ssid.resize((size_t)ns + 1); sc1.resize((size_t)ns + 1);
        st.resize((size_t)n + 1); cov.resize((size_t)n + 1); cov2.resize((size_t)n + 1); conf.resize((size_t)n + 1); abd.resize((size_t)n + 1); scov2.resize((size_t)ns + 1); sconf.resize((size_t)ns + 1); sabd.resize((size_t)ns + 1);
        tid.resize((size_t)n + 1); eo.resize((size_t)n + 2); so.resize((size_t)n + 2);
        return ald_tset_export(t, h.data(), cnt.data(), st.data(), cov.data(), cov2.data(), conf.data(), abd.data(), c1.data(), c2.data(), tid.data(), eo.data(), lr.data(),
                               so.data(), ssid.data(), scov2.data(), sconf.data(), sabd.data(), sc1.data()) == ALD_OK;
    }
    template<class T> static bool same(const std::vector<T> &a, const std::vector<T> &b, size_t k) { return memcmp(a.data(), b.data(), k * sizeof(T)) == 0; }
    bool equals(const flat_set &o) const      // bit for bit
    {
        if(n != o.n || ne != o.ne || ns != o.ns) return false;
        const size_t N = (size_t)n, NE = (size_t)ne, NS = (size_t)ns;
        return same(h, o.h, N) && same(cnt, o.cnt, N) && same(st, o.st, N) && same(cov, o.cov, N) && same(cov2, o.cov2, N) && same(conf, o.conf, N) && same(abd, o.abd, N) && same(c1, o.c1, N) && same(c2, o.c2, N)
            && same(tid, o.tid, N) && same(eo, o.eo, N + 1) && same(lr, o.lr, 2 * NE) && same(so, o.so, N + 1) && same(ssid, o.ssid, NS) && same(scov2, o.scov2, NS) && same(sconf, o.sconf, NS) && same(sabd, o.sabd, NS) && same(sc1, o.sc1, NS);
    }
    typedef std::pair<std::pair<uint64_t, char>, std::vector<int32_t>> key_t;
    // the multi-exon items by (hash, strand, exons); chain_only: by their intron chain -- a merge widens the first exon's left and the
    // last exon's right end (transcript_sink.hpp), so an item made of FEWER transcripts is the same chain with other outer ends
    std::map<key_t, int64_t> multi_exon(bool chain_only = false) const
    {
        std::map<key_t, int64_t> m; const int cut = chain_only ? 1 : 0;
        for(int64_t i = 0; i < n; i++) if(eo[(size_t)i + 1] - eo[(size_t)i] > 1) m[key_t(std::make_pair(h[(size_t)i], st[(size_t)i]), std::vector<int32_t>(lr.begin() + 2 * eo[(size_t)i] + cut, lr.begin() + 2 * eo[(size_t)i + 1] - cut))] = i;
        return m;
    }
};
static bool close12(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::max(std::fabs(a), std::fabs(b)); }
// several submitters: ticket order is the scheduler's, single-exon clusters depend on arrival order -- the multi-exon items must be the
// same set with the same counts and sample ids, sums equal up to the order of the additions
static bool same_up_to_order(const flat_set &got, const flat_set &want, std::string &why)
{
    const std::map<flat_set::key_t, int64_t> g = got.multi_exon(), w = want.multi_exon();
    if(g.size() != w.size()) { why = "multi-exon items: " + std::to_string(g.size()) + " against " + std::to_string(w.size()); return false; }
    for(const auto &kv : w) {
        const auto f = g.find(kv.first); if(f == g.end()) { why = "a multi-exon item is missing"; return false; }
        const size_t a = (size_t)f->second, b = (size_t)kv.second;
        if(got.cnt[a] != want.cnt[b] || got.c2[a] != want.c2[b]) { why = "counts differ"; return false; }
        if(!close12(got.cov[a], want.cov[b]) || !close12(got.cov2[a], want.cov2[b])) { why = "coverage differs beyond the order of additions"; return false; }
        std::vector<int32_t> sa(got.ssid.begin() + got.so[a], got.ssid.begin() + got.so[a + 1]), sb(want.ssid.begin() + want.so[b], want.ssid.begin() + want.so[b + 1]);
        std::sort(sa.begin(), sa.end()); std::sort(sb.begin(), sb.end());
        if(sa != sb) { why = "sample ids differ"; return false; }
    }
    return true;
}

// the serial loop: all items through ONE batch, then one ald_tset_add per graph.  ticket[i]: the ticket item i gets from its queue.
static bool serial_reference(const mock_parameters &cfg, const std::vector<long> &ticket, bool skip, ald_tset *ref)
{
    aletsch::packed_chunk c; aletsch::packed_chunk::scratch tmp; struct { std::map<std::vector<int>, int> nodes; } none;
    for(item &it : items) { if(it.raw) { c.append_graph(*it.g, none, it.sid, tmp); c.last_is_raw(it.px, 10000); } else c.append_graph(*it.g, *it.hs, it.sid, tmp); }
    ald_params p = aletsch::stage_params(cfg); ald_batch *b = nullptr;
    if(ald_batch_create(&p, 0, &b) != ALD_OK) return false;
    bool ok = c.add_to(b) == ALD_OK && ald_batch_upload(b) == ALD_OK && ald_batch_run(b) == ALD_OK && ald_batch_download(b) == ALD_OK;
    for(size_t i = 0; ok && i < items.size(); i++) {
        ald_result_view r; if(ald_batch_get_result(b, (int32_t)i, &r) != ALD_OK) { ok = false; break; }
        std::vector<char> st; std::vector<double> cov, conf, abd; std::vector<int32_t> c1, lr; std::vector<int64_t> tid, eo(1, 0);
        for(int k = 0; k < r.num_paths; k++) {
            ald_transcript_view tv; if(ald_batch_get_transcript(b, (int32_t)i, k, &tv) != ALD_OK) { ok = false; break; }
            st.push_back(tv.strand); cov.push_back(tv.coverage); conf.push_back(tv.conf); abd.push_back(tv.abd); c1.push_back(tv.count1); tid.push_back(((int64_t)ticket[i] << 20) | k);
            lr.insert(lr.end(), tv.exons, tv.exons + 2 * tv.num_exons); eo.push_back(eo.back() + tv.num_exons);
        }
        if(!ok || r.num_paths == 0) continue;
        const int64_t grp[2] = {0, r.num_paths}; const int32_t sid = items[i].sid; lr.push_back(0);
        ok = ald_tset_add(ref, 1, grp, &sid, st.data(), cov.data(), conf.data(), abd.data(), c1.data(), tid.data(), eo.data(), lr.data(), skip ? 1 : 0) == ALD_OK;
    }
    ald_batch_destroy(b);
    return ok;
}

static int fail(const char *what, const std::string &more = std::string()) { printf("FAILED %s %s\n", what, more.c_str()); return 1; }

int main(int argc, char **argv)
{
    if(argc != 5 && argc != 7) { fprintf(stderr, "usage: %s T D P S [ENTRY K]\n", argv[0]); return 2; }
    const int T = atoi(argv[1]), D = atoi(argv[2]), P = atoi(argv[3]), S = atoi(argv[4]);
    const char *entry = argc == 7 ? argv[5] : nullptr; const long kth = argc == 7 ? atol(argv[6]) : 0;
    int N, R;
    if(scanf("%d %d", &N, &R) != 2 || T < 1 || D < 1) return 2;
    std::vector<mock_graph> gs((size_t)(N + R)); std::vector<mock_hyper_set> hs((size_t)(N + R)); mock_parameters cfg;
    for(int n = 0; n < N + R; n++) if(!read_mock_graph(stdin, gs[(size_t)n], hs[(size_t)n])) return 2;
    for(int a = 0, r = 0; a < N || r < R; ) {
        const bool raw = r < R && (items.size() % 5 == 4 || a == N);
        const size_t k = raw ? (size_t)(N + r++) : (size_t)a++;
        item it; it.g = &gs[k]; it.hs = &hs[k]; it.raw = raw; it.sid = (int)(items.size() % 3);
        if(raw) for(const auto &kv : hs[k].nodes) it.px.pmap[std::vector<int32_t>(kv.first.begin(), kv.first.end())] = kv.second;
        items.push_back(it);
    }
    const size_t M = items.size(), cut1 = M / 3, cut2 = 2 * M / 3;
    const std::vector<int> devices = [&] { std::vector<int> d; for(int i = 0; i < D; i++) d.push_back(i); return d; }();
    ald_tset *sink = nullptr, *ref = nullptr;
    if(ald_tset_create(0.8, &sink) != ALD_OK || ald_tset_create(0.8, &ref) != ALD_OK) return 3;
    stub_reset();
    if(D > 1 || entry) stub_set_delay(20261020u, 3);

    if(entry) {
        // ---- error run: one call fails while the submitters are at work; nobody may hang, nothing half merged ----
        const int code = ALD_ERR_HIP;
        stub_inject(entry, kth, code);
        std::atomic<int> returned(0), threw(0), other(0);
        bool drain_threw = false; std::string drain_what; int drain_code = 0;
        {
            queue_t q(cfg, sink, true, devices, 64, S, 8, P);
            std::vector<std::thread> th;
            for(int t = 0; t < T; t++) th.emplace_back([&, t] {
                try { for(size_t i = (size_t)t; i < M; i += (size_t)T) submit_item(q, i); returned++; }
                catch(const aletsch::gpu_error &) { threw++; } catch(...) { other++; }
            });
            for(auto &x : th) x.join();
            try { q.drain(); } catch(const aletsch::gpu_error &e) { drain_threw = true; drain_what = e.what(); drain_code = e.code; }
        }   // the destructor returns
        const std::string text = std::string("injected failure: ") + entry + " call " + std::to_string(kth);
        if(other.load() || returned.load() + threw.load() != T) return fail("a submitter ended with something other than a return or gpu_error");
        if(stub_calls(entry) < kth) return fail("the injected call was never reached");
        if(!drain_threw || drain_code != code || drain_what.find(text) == std::string::npos) return fail("drain() did not throw gpu_error with the injected code and text:", drain_what);
        std::vector<long> ticket(M); for(size_t i = 0; i < M; i++) ticket[i] = (long)i;
        stub_reset();
        if(!serial_reference(cfg, ticket, true, ref)) return fail("serial reference");
        flat_set got, want; if(!got.fetch(sink) || !want.fetch(ref)) return fail("export");
        if(got.n > want.n) return fail("the sink holds more items than a clean run");
        const std::map<flat_set::key_t, int64_t> g = got.multi_exon(true), w = want.multi_exon(true);
        for(const auto &kv : g) {       // whole batches only: an item is a clean run's, made of no more transcripts than there
            const auto f = w.find(kv.first); if(f == w.end()) return fail("the sink holds an intron chain no clean run has");
            if(got.cnt[(size_t)kv.second] > want.cnt[(size_t)f->second]) return fail("an item counts more transcripts than in a clean run");
        }
        printf("CASE error inject=%s call=%ld submitters=%d pack=%d devices=%d slots=%d returned=%d threw=%d items=%lld clean_items=%lld OK\n", entry, kth, T, P, D, S, returned.load(), threw.load(), (long long)got.n, (long long)want.n);
        ald_tset_destroy(sink); ald_tset_destroy(ref);
        return 0;
    }

    // ---- clean run ----
    std::mutex gm; std::condition_variable gcv; int round = 0, done = 0; queue_t *cur = nullptr;      // the gate of the threads that outlive queue A
    std::atomic<int> submitters(0);                                   // threads that handed in at least one graph
    auto share = [&](queue_t &q, int t, size_t lo, size_t hi) { bool any = false; for(size_t i = lo + (size_t)t; i < hi; i += (size_t)T) { submit_item(q, i); any = true; } return any; };
    std::vector<std::thread> old;
    thread_probe_reset();
    for(int t = 0; t < T; t++) old.emplace_back([&, t] {
        bool any = false;
        for(int r : {1, 3}) {
            queue_t *q; { std::unique_lock<std::mutex> lk(gm); gcv.wait(lk, [&] { return round >= r; }); q = cur; }
            any = share(*q, t, r == 1 ? 0 : cut2, r == 1 ? cut1 : M) || any;
            { std::lock_guard<std::mutex> lk(gm); done++; } gcv.notify_all();
        }
        if(any) submitters++;
    });
    auto run_round = [&](queue_t *q, int r) {
        { std::lock_guard<std::mutex> lk(gm); cur = q; round = r; done = 0; } gcv.notify_all();
        std::unique_lock<std::mutex> lk(gm); gcv.wait(lk, [&] { return done == T; });
    };
    long batches = 0, failed = 0, queue_threads = 0;
    try {
        std::unique_ptr<queue_t> q;
        { const long s0 = thread_probe().started; q.reset(new queue_t(cfg, sink, false, devices, 64, S, 8, P)); queue_threads = thread_probe().started - s0; }
        run_round(q.get(), 1); q->drain();
        if(q->submitted() != (long)cut1) return fail("round 1: submitted() is not the number of graphs handed in");
        { std::vector<std::thread> fresh; for(int t = 0; t < T; t++) fresh.emplace_back([&, t] { if(share(*q, t, cut1, cut2)) submitters++; }); for(auto &x : fresh) x.join(); }
        q->drain(); q->drain();
        if(q->submitted() != (long)cut2) return fail("round 2: submitted() is not the number of graphs handed in");
        batches += q->batches(); failed += q->failed_graphs();
        q.reset();                                                     // queue A is gone; its submitting threads live on
        q.reset(new queue_t(cfg, sink, false, devices, 64, S, 8, P));
        run_round(q.get(), 3); q->drain();
        if(q->submitted() != (long)(M - cut2)) return fail("round 3: the second queue did not start its tickets at 0");
        batches += q->batches(); failed += q->failed_graphs();
    } catch(const std::exception &e) { return fail("EXCEPTION", e.what()); }
    for(auto &x : old) x.join();
    const int sink_width = stub_sink_width_min(), stage_width = stub_stage_width_max();

    std::vector<long> ticket(M); for(size_t i = 0; i < M; i++) ticket[i] = (long)(i < cut2 ? i : i - cut2);      // one submitter: tickets are the submission order of each queue
    stub_reset();
    if(!serial_reference(cfg, ticket, false, ref)) return fail("serial reference");
    flat_set got, want; if(!got.fetch(sink) || !want.fetch(ref)) return fail("export");
    if(want.n < 100) return fail("the graph set gives too few transcripts to mean anything");
    std::string why;
    if(T == 1 ? !got.equals(want) : !same_up_to_order(got, want, why)) return fail(T == 1 ? "the sink is not, bit for bit, the serial loop's" : "the sink differs from the serial loop's:", why);
    printf("CASE clean submitters=%d queue_threads=%ld pack=%d devices=%d slots=%d sink=%d staging=%d batches=%ld failed=%ld items=%lld OK\n",
           submitters.load(), queue_threads, P, D, S, sink_width, stage_width, batches, failed, (long long)got.n);
    ald_tset_destroy(sink); ald_tset_destroy(ref);
    return 0;
}
