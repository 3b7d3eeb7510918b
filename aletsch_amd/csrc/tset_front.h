// tset_front.h -- what the two transcript-set translation units share: the device front end of a batch's transcripts (tset_reduce.hip)
// and the record / flat-set types both sides read.  tset_reduce.hip folds a batch into an EMPTY set (row f3); tset_resident.hip folds it
// into a set that stays in HBM across calls.  Not installed, not part of the ABI.
#pragma once
#include "ald_internal.h"
#include "tset_flat.h"          // ald_tset_flat, its column view and row operations
#include <string>
#include <vector>

#define HCHK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) return ald_set_err(ALD_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while(0)

enum { TX_BLOCK = 256 };
static const uint64_t TX_HOST = ~0ull;                 // key of a transcript the host merges (fewer than two exons)
inline unsigned grid_for(int64_t n) { return (unsigned)((n + TX_BLOCK - 1) / TX_BLOCK); }

// The paths of a batch as the kernels see them: record offsets in (graph, path) order + the record pool.  A record carries the joined
// exons of its transcript behind the vertex list (record_layout.h), written by the decomposition kernel, so nothing here needs the
// staged graphs or a host-side parse.
struct TxIn { const unsigned long long *roff; const uint32_t *pool; int64_t np; };

// transcript::get_intron_chain_hashing (transcript.cc:183-201, util.cc:38-46) over the flat exon words; 64-bit size_t arithmetic as on the host
__host__ __device__ inline uint64_t chain_key_dev(const int32_t *x, int n_words)
{
    uint64_t h = (uint64_t)(n_words - 2);
    for(int k = 1; k + 1 < n_words; k++) h ^= (uint64_t)(int64_t)x[k] + 0x9e3779b9ull + (h << 6) + (h >> 2);
    return (h & 0x7FFFFFFFull) + 1;
}
// the bucket of ANY transcript, as transcript_sink::chain_key has it: no exon -> 0, one exon -> its mid-point bin in int32 arithmetic
__host__ __device__ inline uint64_t bucket_key_dev(const int32_t *x, int n_words)
{
    if(n_words < 2) return 0;
    if(n_words == 2) return (uint64_t)(int64_t)((x[0] + x[1]) / 10000) + 1;
    return chain_key_dev(x, n_words);
}

// first: path (in (graph, path) order) whose record the item takes its exons, strand and id from
struct TxGroup { int64_t first; unsigned long long first_off; int32_t count, count1, lo, hi; double coverage, cov2, conf, abd; uint32_t bucket; int32_t nw, graph, path, strand, pad; };
// one (group, sample) run: the per-sample maxima of a group's members from one sample
struct TxSample { int32_t gid, sid, count1, pad; double cov2, conf, abd; };

// scratch of a front end run (owned by a batch or a resident set and kept across calls, or temporary for the stream entry point)
// d2h (optional): every byte the front end copies device -> host is added to it (ald_tset_dev_stream_stats)
struct RedScratch { TxScratch *x; hipStream_t st; int64_t *d2h = nullptr; };
inline void tx_count_d2h(const RedScratch &S, size_t bytes) { if(S.d2h) *S.d2h += (int64_t)bytes; }
// what a temporary owner holds for one call: scratch (anything with release()), a stream, a pair of events -- gone on scope exit
template<class T> struct Scoped : T { ~Scoped() { this->release(); } };
struct ScopedStream { hipStream_t s = nullptr; ~ScopedStream() { if(s) hipStreamDestroy(s); } };
struct EventPair { hipEvent_t a = nullptr, b = nullptr; ~EventPair() { if(a) hipEventDestroy(a); if(b) hipEventDestroy(b); } };
// a visible HIP device of that index, or the error an entry point returns without one.  who: the caller's noun ("the reduction")
inline int tx_need_device(int32_t device, const char *who)
{
    int ndev = 0;
    if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ald_set_err(ALD_ERR_NO_DEVICE, std::string("no HIP device visible: ") + who + " has no CPU fallback");
    if(device < 0 || device >= ndev) return ald_set_err(ALD_ERR_INVALID, "device index out of range");
    return ALD_OK;
}
// The hipCUB two-step: call(null, bytes) asks for the temporary storage, tmp grows to it, call(tmp.p, bytes) enqueues the work.
// call(void *tmp, size_t &bytes) -> hipError_t.  A growth of tmp frees the old block, which waits for the device: safe between enqueued
// work, and it only happens on an input larger than any before.
template<class F> int tx_cub(DevBuf &tmp, const char *what, F call)
{
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if(e == hipSuccess) { if(tmp.ensure(bytes + 256)) return ald_set_err(ALD_ERR_NOMEM, what); e = call(tmp.p, bytes); }
    return e == hipSuccess ? ALD_OK : ald_set_err(ALD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// is p device memory?  (a plain host pointer makes the query fail: not an error here)
inline bool tx_on_device(const void *p)
{
    hipPointerAttribute_t at; const bool dev = p && hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    return dev;
}

// What the front end leaves behind: TxScratch's cov, weight, key_sorted, sidx, head, gid, groups, samples (ald_internal.h says what each
// holds).  host_paths: the transcripts with fewer than two exons, (graph, path) order.
// ev0 (optional): recorded once the inputs are on the device, i.e. where the device time of the caller's section begins.
// ev_w / h_cov: only when the coverages are made from the records (tx_front_sort without h_cov): the event behind the D2H of the weights,
// and the coverages tx_front_coverage computed (pinned, p_cov).
// d_cov (set by the caller, optional): coverage per path already in DEVICE memory (a device stream folded with the caller's coverages):
// tx_front_sort without h_cov then copies it device to device and neither fetches the weights nor needs tx_front_coverage.
struct TxFront { int64_t np = 0, n_dev = 0; int32_t n_groups = 0, n_runs = 0; std::vector<int64_t> host_paths; hipEvent_t ev0 = nullptr; bool sid_on_device = false;
                 hipEvent_t ev_w = nullptr; const double *h_cov = nullptr; const double *d_cov = nullptr; };
inline const uint64_t *tx_skey(const RedScratch &S) { return (const uint64_t*)S.x->key_sorted.p; }
inline const int64_t *tx_sidx(const RedScratch &S) { return (const int64_t*)S.x->sidx.p; }
inline const int32_t *tx_head(const RedScratch &S) { return (const int32_t*)S.x->head.p; }
inline const int32_t *tx_gid(const RedScratch &S) { return (const int32_t*)S.x->gid.p; }
inline TxGroup *tx_groups(const RedScratch &S) { return (TxGroup*)S.x->groups.p; }
inline TxSample *tx_samples(const RedScratch &S) { return (TxSample*)S.x->samples.p; }

// exon join / bucket hash / stable sort by group / head flags / group ids: F.n_dev, F.n_groups, F.host_paths.  h_cov: coverage per path
// (host libm), sid: sample per graph or null.  Enqueued on S.st; returns after the counts are on the host.
int tx_front_groups(RedScratch S, TxIn in, const double *h_cov, int n_graphs, const int32_t *sid, TxFront &F);
// tx_front_groups in its two halves, for a caller without a host copy of the records (a batch that ald_batch_finish ended):
//   tx_front_sort      keys + the stable sort, ENQUEUED only.  h_cov = null: the key pass also writes weight[p] (ALD_REC_WEIGHT) into a dense
//                      array in (graph, path) order (weight), 8 bytes per path go to pinned memory (p_weight) and F.ev_w is recorded
//   tx_front_coverage  waits for F.ev_w, takes log(1 + w) with the host's libm on up to 16 threads (ALD_SINK_THREADS) WHILE THE SORT RUNS, and
//                      enqueues the upload to where tx_front_groups puts h_cov (cov): coverage is first read by tx_fold
//   tx_front_heads     waits for the sort; head flags, group ids, F.n_dev / n_groups / host_paths
int tx_front_sort(RedScratch S, TxIn in, const double *h_cov, int n_graphs, const int32_t *sid, TxFront &F);
int tx_front_coverage(RedScratch S, TxFront &F);
int tx_front_heads(RedScratch S, TxIn in, TxFront &F);
// The records of F.host_paths (fewer than two exons) compacted on the device -- lengths, exclusive scan, a 16-lane copy per record into
// d_out -- and brought to pinned memory (p_single_off, p_single_words): *h_words + (*h_off)[a] is the record of F.host_paths[a].
// Enqueued on S.st; the caller waits for the stream before it reads them.
int tx_compact_singles(RedScratch S, TxIn in, const TxFront &F, DevBuf &d_out, const uint32_t **h_words, const unsigned long long **h_off);
// the fold of every group (tx_fold) and its per-sample runs (tx_sfold).  start_idx[group] >= 0: the group lands on a resident item whose
// coverage start_cov[start_idx[group]] the group's graphs add to, one by one ((c + s1) + s2) + ...; null: every group starts empty.
int tx_front_fold(RedScratch S, TxIn in, TxFront &F, const int64_t *start_idx, const double *start_cov);
// the transcripts with fewer than two exons into `into`, graph by graph (one per-graph set per graph, assembler.cc:1105-1133)
// h_off (optional): the record of host_paths[a] lies at h_pool + h_off[a] (tx_compact_singles) instead of h_pool + h_roff[host_paths[a]]
void tx_host_singles(aletsch::transcript_sink &into, const std::vector<int64_t> &host_paths, const uint32_t *h_pool, const unsigned long long *h_roff,
                     const double *h_cov, const int64_t *h_tid, const int32_t *sid, const int64_t *label, int64_t tid_base, const unsigned long long *h_off = nullptr);
// a transcript stream (format of ald_batch_transcript_stream) turned into records the front end reads
struct StreamRecords { std::vector<uint32_t> pool; std::vector<unsigned long long> roff; std::vector<double> cov; std::vector<int32_t> sid; std::vector<int64_t> label, tids; int64_t n_transcripts = 0; };
int tx_stream_records(const uint32_t *words, int64_t n_words, const double *coverage, const int64_t *tid, int32_t skip_single_exon, int64_t graph_offset, StreamRecords &R);
// The host walk over the transcript boundaries of a stream: each(o, first) for the transcript at word o, first = it begins a run of equal
// graph ids.  A header or record that does not fit, a negative exon count, a descending graph id: ALD_ERR_INVALID.
template<class F> int tx_walk_stream(const uint32_t *words, int64_t n_words, F each)
{
    int64_t last = -1;
    for(int64_t o = 0; o < n_words; ) {
        if(o + ALD_TS_HDR > n_words) return ald_set_err(ALD_ERR_INVALID, "malformed transcript stream");
        const uint32_t *w = words + o; const int64_t len = ts_words(w);
        if((int32_t)w[ALD_TS_NEXONS] < 0 || o + len > n_words) return ald_set_err(ALD_ERR_INVALID, "malformed transcript stream");
        const int64_t g = (int64_t)w[ALD_TS_GRAPH];
        if(g < last) return ald_set_err(ALD_ERR_INVALID, "transcript stream not in ascending graph order");
        each(o, g != last);
        last = g; o += len;
    }
    return ALD_OK;
}
// The same walk on the device (tset_index.hip): the transcript boundaries of a stream in DEVICE memory by pointer doubling over the record
// lengths.  toff[i] = first word of transcript i, toff[nt] = n_words; gid[i] = 1-based run of equal graph ids transcript i belongs to
// (runs counted before any single-exon filter, as tx_stream_records pushes label / sid before it skips); label[k] = graph id of run k +
// graph_offset, sid[k] = ALD_TS_SID of its first transcript.  All four live in X (the caller's) until the next call.
// Kernels on `st`; ONE copy of 40 bytes (counts + flags, into X.p_sum) and one synchronisation.  e0 / e1 (optional): recorded around the
// kernels, ms = the time between them.  Malformed or descending: ALD_ERR_INVALID as tx_stream_records; n_words == 0 launches nothing;
// n_words >= 2^31: ALD_ERR_INVALID (the callers keep the host walk for such a stream).
struct StreamIndex { const unsigned long long *toff = nullptr; const int32_t *gid = nullptr; const int64_t *label = nullptr; const int32_t *sid = nullptr; int64_t nt = 0, ng = 0; double ms = 0; };
int tx_stream_index(hipStream_t st, StreamIndexScratch &X, hipEvent_t e0, hipEvent_t e1, const uint32_t *d_words, int64_t n_words, int64_t graph_offset, StreamIndex &I);
// the path table of a downloaded or finished batch in (graph, path) order on the device (b->d_ordoff), built once per run
int device_path_table(ald_batch *b);
