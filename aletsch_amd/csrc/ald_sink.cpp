// ald_sink.cpp -- the host result sink of the C ABI (include/aletsch_decomp.h: ald_tset_*) and the finished-transcript stream of a
// downloaded batch.  Plain host code: it reads a batch's decoded results (HostResults) and the shard tables, and makes no HIP call --
// a translation unit of its own so that a CPU program can link it as it is next to a stand-in for the batch entry points
// (tests/host_adapter/stub_batch_abi.cc: the threaded passes below run under ThreadSanitizer there).
#include "ald_internal.h"
#include "tset_front.h"          // tx_walk_stream
#include <thread>
#include <chrono>
#include <string>
#include <cstdlib>
#include <cstdio>
#include <cmath>

namespace { inline int set_err(int code, const std::string &s) { return ald_set_err(code, s); } }

extern "C" {

/* ---- result sink: transcript_set restated (aletsch_amd/host/transcript_sink.hpp) ---- */

int ald_tset_create(double single_exon_overlap, ald_tset **out) { if(!out) return ALD_ERR_INVALID; *out = new ald_tset(single_exon_overlap); return ALD_OK; }
int ald_tset_destroy(ald_tset *t) { delete t; return ALD_OK; }

int ald_tset_add(ald_tset *t, int32_t n_groups, const int64_t *group_offset, const int32_t *group_sid,
                 const char *strand, const double *coverage, const double *conf, const double *abd, const int32_t *count1,
                 const int64_t *tid, const int64_t *exon_offset, const int32_t *exon_lr, int32_t skip_single_exon)
{
    if(!t || n_groups < 0 || (n_groups > 0 && (!group_offset || !group_sid || !strand || !coverage || !conf || !abd || !count1 || !tid || !exon_offset || !exon_lr))) return ALD_ERR_INVALID;
    for(int g = 0; g < n_groups; g++) {
        aletsch::transcript_sink ts(t->overlap);
        for(int64_t i = group_offset[g]; i < group_offset[g + 1]; i++) {
            aletsch::sink_transcript x;
            x.strand = strand[i]; x.coverage = coverage[i]; x.top.cov2 = coverage[i]; x.top.conf = conf[i]; x.top.abd = abd[i]; x.top.count1 = count1[i]; x.count2 = 1; x.tid = tid[i];
            x.xs.assign(exon_lr + 2 * exon_offset[i], exon_lr + 2 * exon_offset[i + 1]);
            if(x.n_exons() <= 1 && skip_single_exon) continue;               // assembler.cc:1117
            ts.add(x, 1, group_sid[g]);                                      // assembler.cc:1120
        }
        t->add(ts);                                                          // assembler.cc:1130
    }
    return ALD_OK;
}

} // extern "C"  (the helpers below are templates / C++ types)
namespace {
unsigned sink_threads(int64_t n_transcripts)
{
    unsigned nthr = std::thread::hardware_concurrency(); if(nthr == 0) nthr = 1; if(nthr > 16) nthr = 16;
    if(const char *ev = getenv("ALD_SINK_THREADS")) { int k = atoi(ev); if(k >= 1 && k <= 64) nthr = (unsigned)k; }
    else if(n_transcripts < 20000) nthr = 1;
    if(nthr > ALD_TSET_SHARDS) nthr = ALD_TSET_SHARDS;
    return nthr;
}
} unsigned ald_sink_threads(int64_t n_items) { return sink_threads(n_items); } namespace {
const uint32_t ALD_NO_BUCKET = 0xFFFFFFFFu;       // hashes are below 2^31 + 1

// The merge of many graphs' transcripts.  Buckets never interact, so they are dealt to the host threads by hash: every thread walks
// the groups (graphs) in ascending order, builds the per-graph set of ITS buckets and merges it -- the same sequence of
// trans_item::merge calls per bucket as the serial loop of assembler.cc:1105-1133, hence the same result, without `mylock`.
// `make(i, x)` fills x from transcript i; grp[k] .. grp[k+1] are the transcripts of group k; bucket[i] = its chain key or ALD_NO_BUCKET.
struct no_prefetch { void operator()(int64_t) const {} };
template<class Make, class Pre = no_prefetch> void merge_groups(ald_tset *t, unsigned nthr, int64_t n_groups, const int64_t *grp, const int32_t *grp_sid, const uint32_t *bucket, Make make, Pre pre = Pre())
{
    // the transcripts are dealt to their owners first (a counting sort by owner over contiguous ranges, so that every owner's list is in
    // ascending (graph, path) order): an owner then walks its own sixteenth instead of testing every transcript of the batch
    const int64_t nt = n_groups > 0 ? grp[n_groups] : 0;
    auto owner = [&](uint32_t h) { return (unsigned)((h % ALD_TSET_SHARDS) % nthr); };
    std::vector<int64_t> base((size_t)nthr * nthr, 0), first((size_t)nthr + 1, 0);
    HostBatch::run_threads(nthr, [&](unsigned r) {
        int64_t *c = &base[(size_t)r * nthr];
        for(int64_t i = nt * r / nthr; i < nt * (r + 1) / nthr; i++) if(bucket[(size_t)i] != ALD_NO_BUCKET) c[owner(bucket[(size_t)i])]++;
    });
    for(unsigned o = 0; o < nthr; o++) { int64_t run = first[o]; for(unsigned r = 0; r < nthr; r++) { const int64_t c = base[(size_t)r * nthr + o]; base[(size_t)r * nthr + o] = run; run += c; } first[(size_t)o + 1] = run; }
    std::vector<int64_t> order((size_t)first[nthr]);
    HostBatch::run_threads(nthr, [&](unsigned r) {
        int64_t *c = &base[(size_t)r * nthr];
        for(int64_t i = nt * r / nthr; i < nt * (r + 1) / nthr; i++) if(bucket[(size_t)i] != ALD_NO_BUCKET) order[(size_t)c[owner(bucket[(size_t)i])]++] = i;
    });
    HostBatch::run_threads(nthr, [&](unsigned th) {
        aletsch::sink_transcript x;
        int64_t g = 0;
        // the loop is bound by cache misses (source record -> index slot -> table entry): what transcript k + 12 / k + 8 / k + 4 will touch is
        // asked for while transcript k is merged
        const int64_t end = first[(size_t)th + 1];
        static const int dist[3] = { getenv("ALD_SINK_AHEAD_REC") ? atoi(getenv("ALD_SINK_AHEAD_REC")) : 12, getenv("ALD_SINK_AHEAD_SLOT") ? atoi(getenv("ALD_SINK_AHEAD_SLOT")) : 8,
                                     getenv("ALD_SINK_AHEAD_ENTRY") ? atoi(getenv("ALD_SINK_AHEAD_ENTRY")) : 4 };      // tuning knobs (0 = off)
        auto ahead = [&](int64_t k) {
            if(dist[0] > 0 && k + dist[0] < end) pre(order[(size_t)(k + dist[0])]);
            if(dist[1] > 0 && k + dist[1] < end) { const uint32_t h = bucket[(size_t)order[(size_t)(k + dist[1])]]; t->shard[h % ALD_TSET_SHARDS].mt.prefetch_slot(h); }
            if(dist[2] > 0 && k + dist[2] < end) { const uint32_t h = bucket[(size_t)order[(size_t)(k + dist[2])]]; t->shard[h % ALD_TSET_SHARDS].mt.prefetch_entry(h); }
        };
        for(int64_t k = first[th]; k < end; ) {
            while(grp[g + 1] <= order[(size_t)k]) g++;                           // the graph of this owner's next transcript
            int64_t k1 = k; while(k1 < end && order[(size_t)k1] < grp[g + 1]) k1++;
            const int64_t *idx = &order[(size_t)k]; const int cnt = (int)(k1 - k);
            for(int64_t q = k; q < k1; q++) ahead(q);
            k = k1;
            const int s_id = grp_sid ? grp_sid[g] : -1;
            // a graph that puts a single transcript into this thread's tables needs no per-graph set: merging a one-item set is the same
            // as adding the item (transcript_set.cc:149-175)
            if(cnt == 1) { make(idx[0], x); const uint32_t h = bucket[(size_t)idx[0]]; t->shard[h % ALD_TSET_SHARDS].add_hashed(x, h, 1, s_id); continue; }
            // ... and so is merging a set whose items all sit in DIFFERENT buckets: transcript_set::add(set) goes bucket by bucket
            // (transcript_set.cc:156-175), and a bucket that receives one item is zipped exactly as add() would place that item.  Only
            // transcripts of one graph that share a bucket (equal intron chains, single-exon clusters) need the graph's own set first.
            if(cnt <= 16) {
                bool distinct = true;
                for(int a = 1; a < cnt && distinct; a++) for(int q = 0; q < a && distinct; q++) distinct = bucket[(size_t)idx[q]] != bucket[(size_t)idx[a]];
                if(distinct) { for(int q = 0; q < cnt; q++) { make(idx[q], x); const uint32_t h = bucket[(size_t)idx[q]]; t->shard[h % ALD_TSET_SHARDS].add_hashed(x, h, 1, s_id); } continue; }
            }
            aletsch::transcript_sink ts(t->overlap);
            for(int q = 0; q < cnt; q++) {
                make(idx[q], x);
                ts.add_hashed(x, bucket[(size_t)idx[q]], 1, s_id);              // assembler.cc:1120
            }
            t->add(ts);                                                        // assembler.cc:1130 (only tables this thread owns are touched)
        }
    });
}

} // namespace

extern "C" {
int ald_tset_add_batch(ald_tset *t, const ald_batch *b, const int32_t *sid, int64_t tid_base, int32_t skip_single_exon)
{
    if(!t || !b || !b->downloaded) return ALD_ERR_INVALID;
    auto T0 = std::chrono::steady_clock::now();
    const int n = b->hb.n();
    const int64_t np = b->res.n_paths();
    const unsigned nthr = sink_threads(np);
    // pass 1: bucket of every transcript -- the key was taken by the download while it decoded the record (HostResults::build)
    std::vector<uint32_t> bucket((size_t)np, ALD_NO_BUCKET);
    HostBatch::run_threads(nthr, [&](unsigned th) {
        for(int64_t i = np * th / nthr; i < np * (th + 1) / nthr; i++)
            if(!(b->res.n_exon_words[(size_t)i] <= 2 && skip_single_exon)) bucket[(size_t)i] = b->res.chain_key[(size_t)i];      // assembler.cc:1117
    });
    auto T2 = std::chrono::steady_clock::now();
    // pass 2: thread th owns the tables th, th + nthr, ...
    merge_groups(t, nthr, n, b->res.path_begin.data(), sid, bucket.data(), [&](int64_t i, aletsch::sink_transcript &x) {
        const PathRec p = b->res.path((int64_t)((size_t)i));
        x.strand = p.strand; x.coverage = p.coverage; x.top.cov2 = x.coverage; x.top.conf = p.conf; x.top.abd = p.abd; x.top.count1 = p.count; x.count2 = 1;
        x.tid = transcript_tid(tid_base, (int64_t)p.graph, (int64_t)p.index);
        const int32_t *ex = b->res.exons(p);
        x.xs.assign(ex, ex + p.nexw);
    }, [&](int64_t i) { __builtin_prefetch(b->res.rec(i)); __builtin_prefetch(b->res.rec(i) + 16); });
    if(getenv("ALD_SINK_PROF")) { auto T3 = std::chrono::steady_clock::now(); auto ms = [](auto a, auto b2) { return std::chrono::duration<double, std::milli>(b2 - a).count(); }; fprintf(stderr, "[sink] hash pass %.1f ms, merge pass %.1f ms (%u threads)\n", ms(T0, T2), ms(T2, T3), nthr); }
    return ALD_OK;
}

/* ---- finished transcripts as ONE self-contained stream: what ranks exchange in the multi-GPU gather and what a device list merges ----
 * 4-byte words, transcripts in ascending (graph, path index) order:
 *   [graph, path, sid, strand, count1, n_exons, weight f64, conf f64, abd f64, (l, r) * n_exons]        ALD_TS_HDR + 2 * n_exons words (record_layout.h)
 * Records of abandoned attempts and of graphs that did not end well are already gone (HostResults::build), exons are joined. */
int ald_batch_transcript_stream(const ald_batch *cb, const int32_t *sid, int32_t skip_single_exon, const uint32_t **words, int64_t *n_words)
{
    if(!cb || !words || !n_words) return ALD_ERR_INVALID;
    if(!cb->downloaded) return set_err(ALD_ERR_STATE, "ald_batch_transcript_stream before ald_batch_download");
    ald_batch *b = const_cast<ald_batch*>(cb);
    const int64_t np = b->res.n_paths();
    const unsigned nthr = sink_threads(np);
    std::vector<int64_t> at((size_t)np + 1, 0);
    for(int64_t i = 0; i < np; i++) { const int k = (int)b->res.rec(i)[ALD_REC_NEXW]; at[(size_t)i + 1] = at[(size_t)i] + ((k <= 2 && skip_single_exon) ? 0 : ALD_TS_HDR + k); }
    b->tstream.resize((size_t)at[(size_t)np] + 2);
    uint32_t *out = b->tstream.data();
    HostBatch::run_threads(nthr, [&](unsigned th) {
        for(int64_t i = np * th / nthr; i < np * (th + 1) / nthr; i++) {
            if(at[(size_t)i + 1] == at[(size_t)i]) continue;
            const uint32_t *r = b->res.rec(i); uint32_t *w = out + at[(size_t)i];
            for(int l = 0; l < ALD_TS_HDR; l++) w[l] = ts_header_word(r, l, sid);
            if(r[ALD_REC_NEXW]) memcpy(w + ALD_TS_HDR, rec_exons(r), 4 * (size_t)r[ALD_REC_NEXW]);
        }
    });
    *words = out; *n_words = at[(size_t)np];
    return ALD_OK;
}

int ald_tset_add_stream(ald_tset *t, const uint32_t *words, int64_t n_words, int32_t graph_offset, int64_t tid_base)
{
    if(!t || n_words < 0 || (n_words > 0 && !words)) return ALD_ERR_INVALID;
    const auto T0 = std::chrono::steady_clock::now();
    // record boundaries and groups (one serial walk: the lengths are in the records)
    std::vector<int64_t> offs, grp; std::vector<int32_t> grp_sid;
    { int rc = tx_walk_stream(words, n_words, [&](int64_t o, bool first) {
          if(first) { grp.push_back((int64_t)offs.size()); grp_sid.push_back((int32_t)words[o + ALD_TS_SID]); }
          offs.push_back(o);
      }); if(rc != ALD_OK) return rc; }
    const int64_t nt = (int64_t)offs.size(); grp.push_back(nt);
    const unsigned nthr = sink_threads(nt);
    const auto T1 = std::chrono::steady_clock::now();
    std::vector<uint32_t> bucket((size_t)nt);
    HostBatch::run_threads(nthr, [&](unsigned th) {
        for(int64_t i = nt * th / nthr; i < nt * (th + 1) / nthr; i++) { const uint32_t *w = words + offs[(size_t)i]; bucket[(size_t)i] = (uint32_t)aletsch::sink_transcript::chain_key(ts_exons(w), (size_t)ts_nexw(w)); }
    });
    const auto T2 = std::chrono::steady_clock::now();
    merge_groups(t, nthr, (int64_t)grp_sid.size(), grp.data(), grp_sid.data(), bucket.data(), [&](int64_t i, aletsch::sink_transcript &x) {
        const uint32_t *w = words + offs[(size_t)i];
        x.strand = (char)w[ALD_TS_STRAND]; x.coverage = log(1.0 + ts_f64(w, ALD_TS_WEIGHT)); x.top.cov2 = x.coverage; x.top.conf = ts_f64(w, ALD_TS_CONF); x.top.abd = ts_f64(w, ALD_TS_ABD); x.top.count1 = (int32_t)w[ALD_TS_COUNT1]; x.count2 = 1;
        x.tid = transcript_tid(tid_base, (int64_t)w[ALD_TS_GRAPH] + graph_offset, (int64_t)w[ALD_TS_PATH]);
        x.xs.assign(ts_exons(w), ts_exons(w) + ts_nexw(w));
    }, [&](int64_t i) { const uint32_t *w = words + offs[(size_t)i]; __builtin_prefetch(w); __builtin_prefetch((const char*)w + 64); });
    if(getenv("ALD_SINK_PROF")) { const auto T3 = std::chrono::steady_clock::now(); auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) { return std::chrono::duration<double, std::milli>(c - a).count(); };
        fprintf(stderr, "[sink] stream of %lld transcripts: boundaries %.1f ms, hash pass %.1f ms, merge pass %.1f ms (%u threads)\n", (long long)nt, ms(T0, T1), ms(T1, T2), ms(T2, T3), nthr); }
    return ALD_OK;
}

int ald_tset_merge(ald_tset *dst, ald_tset *src)
{
    if(!dst || !src || dst == src) return ALD_ERR_INVALID;
    for(auto &sh : src->shard) { dst->add(sh); sh.clear(); }
    return ALD_OK;
}

int ald_tset_size(const ald_tset *t, int64_t *n_items, int64_t *n_exons, int64_t *n_samples)
{
    if(!t) return ALD_ERR_INVALID;
    int64_t a = 0, e = 0, s = 0;
    for(auto &sh : t->shard) for(auto &x : sh.mt) for(auto &z : x.second) { a++; e += (int64_t)z.trst.n_exons(); s += (int64_t)z.samples.size(); }
    if(n_items) *n_items = a; if(n_exons) *n_exons = e; if(n_samples) *n_samples = s;
    return ALD_OK;
}

int ald_tset_export(const ald_tset *t, uint64_t *hash, int32_t *count, char *strand, double *coverage, double *cov2, double *conf, double *abd,
                    int32_t *count1, int32_t *count2, int64_t *tid, int64_t *exon_offset, int32_t *exon_lr,
                    int64_t *sample_offset, int32_t *sample_sid, double *sample_cov2, double *sample_conf, double *sample_abd, int32_t *sample_count1)
{
    if(!t) return ALD_ERR_INVALID;
    const SinkRows rows = sink_rows(t->shard.data(), t->shard.size());                                  // the reference's iteration order: ascending hash
    const FlatMut out{hash, count, strand, coverage, cov2, conf, abd, count1, count2, tid, exon_offset, exon_lr, sample_offset, sample_sid, sample_cov2, sample_conf, sample_abd, sample_count1, (int64_t)rows.item.size(), rows.ne, rows.ns};
    if(flat_has_null(out)) return ALD_ERR_INVALID;
    exon_offset[0] = sample_offset[0] = 0;
    for(int64_t i = 0; i < out.n; i++) flat_put_item(out, i, rows.hash[(size_t)i], *rows.item[(size_t)i]);
    return ALD_OK;
}

} // extern "C"
