// ald_internal.h -- what the translation units of the host library share: the batch object behind the opaque `ald_batch` handle.
// Not installed, not part of the ABI (include/aletsch_decomp.h is).
#pragma once
#include <hip/hip_runtime.h>
#include "host_pack.h"
#include "record_layout.h"
#include "../host/transcript_sink.hpp"
#include <mutex>
#include <string>
#include <vector>

using namespace ald;

struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t bytes) { if(bytes <= cap) return 0; if(p) hipFree(p); p = nullptr; cap = 0; size_t want = bytes + bytes / 4 + 256; if(hipMalloc(&p, want) != hipSuccess) return -1; cap = want; return 0; }
    void release() { if(p) hipFree(p); p = nullptr; cap = 0; }
};
struct PinBuf {
    void *p = nullptr; size_t cap = 0;
    // landing: a buffer the copy engine fills and the CPU then READS a lot (record parsing, exon gathers): non-coherent pinned memory is
    // cacheable on the CPU side; visibility is given by the stream synchronisation every reader does first
    int ensure(size_t bytes, bool landing = false) { if(bytes <= cap) return 0; if(p) hipHostFree(p); p = nullptr; cap = 0; size_t want = bytes + bytes / 4 + 256;
        const unsigned flags = landing && !getenv("ALD_PIN_COHERENT") ? hipHostMallocNonCoherent : hipHostMallocDefault;
        if(hipHostMalloc(&p, want, flags) != hipSuccess) return -1; cap = want; return 0; }
    void release() { if(p) hipHostFree(p); p = nullptr; cap = 0; }
};

enum { ALD_SIDE_STREAMS = 6, ALD_SIDE_STREAMS_MAX = 8 };      // five for the large classes + one for classes 0..2 (stage_pass): cfg3 88-89 ms against 93 with three (profiles/r04/x_cfg3_side_streams.txt); a batch of one class (the bench) uses one
// kernel slots of a pass: slot c = the plain build of size class c (staged graphs), slot ALD_NUM_CLASSES + c = its raw build (graphs whose
// pre-steps run on the device); a batch without raw graphs only ever uses the first half
enum { ALD_NUM_SLOTS = 2 * ALD_NUM_CLASSES };     // default / upper bound of the side streams the classes of a pass are dealt to
// one pass of a batch, staged: work lists, kernel arguments, grid sizes, stream assignment (see stage_pass)
struct StagedPass {
    std::vector<int32_t> flat; std::vector<KernelArgs> args;
    int nblk[ALD_NUM_SLOTS]; int order[ALD_NUM_SLOTS]; int stream_of[ALD_NUM_SLOTS]; int nord = 0; size_t tot = 0;
};

// the feature table of the last ald_batch_features_all (trst_features.hip): host rows in pinned memory, valid until the next download / clear
struct FeatTable {
    DevBuf d_rows, d_complete, d_rc, d_scratch, d_x[10];
    DevBuf d_gew, d_gecount, d_gdead, d_glive;     // ALD_FEAT_RAW_ON_DEVICE: the grouped-graph overlay of the raw graphs (weight / count / dead flag per edge of the batch, live edges per graph)
    PinBuf h_rows, h_complete, h_rc;
    std::vector<int64_t> row_begin;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool valid = false; double device_ms = 0, call_ms = 0; int64_t device_graphs = 0, host_graphs = 0, n_rows = 0;
    void release() { DevBuf *d[] = {&d_rows, &d_complete, &d_rc, &d_scratch, &d_gew, &d_gecount, &d_gdead, &d_glive}; for(DevBuf *x : d) x->release(); for(DevBuf &x : d_x) x.release();
                     h_rows.release(); h_complete.release(); h_rc.release(); if(e0) hipEventDestroy(e0); if(e1) hipEventDestroy(e1); e0 = e1 = nullptr; valid = false; }
};

// ---- scratch of the transcript-set side (tset_*.hip), one named buffer per role.  Kept by an owner across calls (a batch, a resident set)
// or temporary for one entry point (tset_front.h: Scoped<>); every struct frees what it holds in release().

// The front end of a batch's transcripts (tset_reduce.hip: tx_front_*).  "per path" = in (graph, path) order, "per place" = in sorted order.
// What a front end run leaves behind for its caller: cov, weight, key_sorted, sidx, head, gid, groups, samples.
// A batch's own (ald_batch::tx) is also borrowed by name, outside any reduction, by device_path_table (cub_tmp), the device transcript
// stream (sid, cub_tmp, p_count) and the owner split (sid): all of them enqueue on ald_batch::stream, which is what orders them against
// the reduction and against each other.
struct TxScratch {
    DevBuf single_len, single_at;      // tx_compact_singles: record length / first word of every single-exon record
    DevBuf cov, weight;                // per path: coverage; the record's weight (only when the coverages are made from the records)
    DevBuf nw, graph;                  // per path: exon words, graph
    DevBuf key;                        // per path: group key.  Second life (tx_front_fold): (group, sample) key per place, unsorted
    DevBuf key_sorted;                 // per place: group key, sorted
    DevBuf idx;                        // per path: its ordinal, the sort's value input.  Second life (tx_front_fold): the (group, sample) keys, sorted
    DevBuf sidx;                       // per place: path
    DevBuf sid;                        // per graph: sample id (the caller's, uploaded)
    DevBuf head, gid;                  // per place: first of its group?  1-based group id
    DevBuf groups;                     // TxGroup[n_groups]
    DevBuf cub_tmp;                    // hipCUB temporary storage (tx_cub)
    DevBuf run_head, run_id;           // per (group, sample)-sorted place: first of its run?  1-based run id
    DevBuf samples;                    // TxSample[n_runs], sorted by group, then sample id
    DevBuf pos, pos_sorted;            // places 0 .. n_dev - 1, and the same in (group, sample) order
    PinBuf p_key, p_groups, p_samples; // host copies: sorted group keys, TxGroup[], TxSample[]
    PinBuf p_count;                    // a few counters (merge path of a resident set; length of a batch's device stream)
    PinBuf p_weight, p_cov;            // per path: weights from the records, the coverages tx_front_coverage makes of them
    PinBuf p_single_off, p_single_words;   // tx_compact_singles: offsets and words of the compacted records
    void release() { DevBuf *d[] = {&single_len, &single_at, &cov, &weight, &nw, &graph, &key, &key_sorted, &idx, &sidx, &sid, &head, &gid, &groups, &cub_tmp, &run_head, &run_id, &samples, &pos, &pos_sorted};
                     PinBuf *p[] = {&p_key, &p_groups, &p_samples, &p_count, &p_weight, &p_cov, &p_single_off, &p_single_words};
                     for(DevBuf *x : d) x->release(); for(PinBuf *x : p) x->release(); }
};
// The merge path of a resident set (tset_resident.hip).  Incoming item = a batch's group or an item of a second set, in (hash, compare1) order.
struct MergeScratch {
    DevBuf ghead, perm;                // per group: head place; groups in (bucket, compare1) order
    DevBuf match, ins, unm, start;     // per incoming item: resident item it lands on or -1, insertion point, 1 = new; per group: match (tx_fold's start)
    DevBuf ub, cnt, shift, rmatch;     // exclusive scan of unm; per resident item: new items placed in front, its inclusive scan, the incoming item landing on it
    DevBuf slot, ecnt, scnt;           // per output item: source, exons, samples
    DevBuf sbeg;                       // per group: first sample run
    DevBuf singles;                    // the compacted single-exon records of a finished batch (tx_compact_singles)
    DevBuf cub_tmp;
    void release() { DevBuf *d[] = {&ghead, &perm, &match, &ins, &unm, &start, &ub, &cnt, &shift, &rmatch, &slot, &ecnt, &scnt, &sbeg, &singles, &cub_tmp}; for(DevBuf *x : d) x->release(); }
};
// A device stream turned into scratch records (tset_resident.hip: sr_len / sr_emit).  Per transcript of the stream unless said otherwise.
struct StreamRecScratch {
    DevBuf len, at, keep, kord;        // words of its record (0: left out), first word, 1 = kept, ordinal among the kept
    DevBuf cov_in, tid_in, cov, tid;   // the caller's coverage / tid by stream ordinal (uploaded), and gathered to the kept ordinal
    DevBuf cub_tmp;
    PinBuf p_head;                     // number of kept transcripts, then label and sid of every group
    void release() { DevBuf *d[] = {&len, &at, &keep, &kord, &cov_in, &tid_in, &cov, &tid, &cub_tmp}; for(DevBuf *x : d) x->release(); p_head.release(); }
};
// The stream index (tset_index.hip: tx_stream_index).  toff, gid, label, sid are its results and live here until the next call.
struct StreamIndexScratch {
    DevBuf succ, succ_next, mark;      // per node: successor (two buffers, swapped every round of doubling), reached from position 0?
    DevBuf toff, head, gid;            // per transcript: first word (+ one entry: n_words), first of its run of equal graph ids?  1-based run
    DevBuf label, sid;                 // per run: graph id + graph_offset, sample id
    DevBuf sum, cub_tmp;               // counts + flags (ix_graphs)
    PinBuf p_sum;
    void release() { DevBuf *d[] = {&succ, &succ_next, &mark, &toff, &head, &gid, &label, &sid, &sum, &cub_tmp}; for(DevBuf *x : d) x->release(); p_sum.release(); }
};
// The owner split (tset_partition.hip).  "sorted" = stable by owner.
struct OwnerSplitScratch {
    DevBuf owner, owner_sorted, ord, ord_sorted;   // per transcript: owner, ordinal; the same sorted
    DevBuf len, len_sorted, place;     // per transcript: words; per sorted place: words of the transcript that lands there, its first word (+ one entry: the total)
    DevBuf offsets, cub_tmp;           // first word of every owner's sub-stream (+ the total)
    DevBuf out;                        // the sub-streams, back to back (the stream entry point uses it only when the caller's buffer is on the host)
    void release() { DevBuf *d[] = {&owner, &owner_sorted, &ord, &ord_sorted, &len, &len_sorted, &place, &offsets, &cub_tmp, &out}; for(DevBuf *x : d) x->release(); }
};

struct ald_batch {
    int device = 0; int n_cus = 0;
    Params prm;
    HostBatch hb{true};                             // its arrays in pinned memory: ald_batch_upload copies them to the device as they are
    HostBatch::Section sec[HostBatch::S_COUNT];
    uint64_t in_bytes = 0;
    hipStream_t stream = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // ald_batch_upload's copies go through a stream of another PRIORITY class: the runtime maps the streams of one priority onto a small
    // pool of hardware queues (GPU_MAX_HW_QUEUES), a queue runs its packets in order, and a batch's 34 input copies (25 ms of DMA) in front
    // of ANOTHER batch's kernel launch on the same queue delayed that kernel by 3-4 ms per step of a pipelined caller
    // (profiles/r04/zc_h2d_inclusive_step.txt).  Streams of a different priority have queues of their own.
    hipStream_t up_stream = nullptr;
    // The RESULTS leave through a stream of a priority class no kernel runs in, for the same reason seen from the other side: four rotating
    // batches own 28 normal-priority streams on 4 queues, so one batch's `stream` shares a queue with the side stream ANOTHER batch's class
    // kernel runs on, and the first small copy issued on `stream` right after the caller launched that kernel -- the 16-byte pool counters:
    // the runtime moves a copy that small with a blit kernel, i.e. through the queue -- waited for all of it (one download in four: 38 ms
    // instead of 0.15, profiles/r15/).  Every D2H copy of end_run / ald_batch_finish / ald_batch_download goes to dl_stream after the host
    // has waited for `stream`; `stream` and the side streams carry memsets, kernels and events only.
    // ALD_DOWNLOAD_STREAM: 2 (default) ONE stream per device in the highest class, shared by the batches (dl_shared: a download then waits
    // for dl_done, its own event, never for the stream); 1 a stream of the batch's own in the lowest class (measured: one batch object in
    // four still waits 36 ms there); 0 or no second priority: `stream`.
    hipStream_t dl_stream = nullptr; hipEvent_t dl_done = nullptr; bool dl_shared = false;
    // the size classes run concurrently on a few side streams.  Not one per class: a process only gets a handful of hardware queues
    // (4 by default) and streams beyond that share them in creation order, which can put the two heaviest classes behind each other
    hipStream_t cstream[ALD_SIDE_STREAMS_MAX] = {}; int n_cstream = ALD_SIDE_STREAMS;
    hipEvent_t cdone[ALD_NUM_SLOTS] = {};
    PinBuf pin_in, pin_out, pin_small, pin_index;          // wire buffer / record landing area / status + counters landing area / the result index
    DevBuf d_in, d_status, d_npaths, d_niters, d_pool, d_poolused, d_trace_n, d_trace_codes, d_trace_vals, d_work, d_counter, d_args;
    DevBuf d_gsid;                                         // compact input with derived sample lists: one sample id per graph (HostBatch::g_sid); not a section of BatchIn
    std::mutex in_csr_mu;                                  // compact input: a host reader of the in-CSR builds it on first use (HostBatch::ensure_in_csr)
    DevBuf d_index, d_gfirst;                              // result index written by the kernel: index[graph_first[g] + p] = pool offset of record (g, p)
    DevBuf d_pbegin, d_ordoff;                             // the same in (graph, path) order, built on the device on demand (tset_reduce.hip: device_path_table)
    uint64_t index_cap = 0; int64_t total_paths = 0; bool paths_on_device = false;
    double dl_ms[4] = {0, 0, 0, 0}; int64_t dl_bytes = 0;   // last download: waiting for the kernel / status + retries / D2H copies / decode (diagnostics)
    DevBuf d_slabs[ALD_NUM_SLOTS];
    int blocks[ALD_NUM_SLOTS] = {};
    int occ[ALD_NUM_SLOTS]; ald_batch() { for(int c = 0; c < ALD_NUM_SLOTS; c++) occ[c] = -1; }
    StagedPass *pass0 = nullptr; bool pass0_on_device = false; std::vector<int32_t> cls0;      // first pass of the uploaded batch, staged at upload time
    uint64_t pool_cap_words = 0;
    int trace_cap = 0;
    bool uploaded = false, ran = false, downloaded = false;
    // ald_batch_finish: the run has ended on the device -- status words read, capacity retries and pool growth done, the per-graph counters on
    // the host -- but no record has left HBM.  path_begin: row prefix of the (graph, path) order, as HostResults::path_begin after a download
    bool finished = false;
    std::vector<int64_t> path_begin;
    uint64_t used_words = 0, used_index = 0;               // record words / index entries the run wrote (clamped to the capacities)
    double fin_ms[2] = {0, 0}; int64_t fin_bytes = 0;      // last finish: waiting for the kernel / status + retries + counters; bytes moved to the host
    double kernel_ms = -1;
    // per-graph scheduling state
    std::vector<int32_t> cls, attempt, status, n_paths, n_iters;
    std::vector<int32_t> trace_n, trace_codes; std::vector<double> trace_vals;
    HostResults res;
    int passes = 0;
    const void *launched_slab[ALD_NUM_SLOTS] = {};      // test hook (ald_batch_debug_slab)
    rvec<uint32_t> tstream;                                // last transcript stream built from this batch (ald_batch_transcript_stream)
    TxScratch tx;                                          // scratch of ald_batch_reduce_transcripts, kept across calls (tset_reduce.hip)
    DevBuf d_ts_len, d_ts_at, d_ts_out;                    // ald_batch_device_transcript_stream: lengths (also device_path_table's) / offsets / the stream itself
    OwnerSplitScratch tp; std::vector<int64_t> tp_offsets; // ald_batch_device_transcript_streams_by_owner (tset_partition.hip): scratch + the sub-streams, their offsets
    FeatTable feat;                                        // ald_batch_features_all
};


// The result sink behind ald_tset_*.  Buckets (intron-chain hashes) never interact: the set is kept as NSHARD independent tables, bucket h
// in table h % NSHARD, so that a whole batch can be merged by NSHARD host threads without a lock; the export walks all keys in ascending order.
enum { ALD_TSET_SHARDS = 16 };
struct ald_tset {
    std::vector<aletsch::transcript_sink> shard; double overlap;
    explicit ald_tset(double ov) : shard(ALD_TSET_SHARDS, aletsch::transcript_sink(ov)), overlap(ov) {}
    void add(aletsch::transcript_sink &ts) { for(auto &x : ts.mt) shard[x.first % ALD_TSET_SHARDS].add_bucket(x.first, x.second); }
};

unsigned ald_sink_threads(int64_t n_items);          // host threads for a merge of n items (ALD_SINK_THREADS overrides; at most one per table)
int ald_ensure_index(const ald_batch *b);                 // per-graph index over the record stream of the last download (built on first use)
int ald_expand_input(const ald_batch *b, hipStream_t st);  // compact input (input_expand.hip): enqueues the kernels that fill the sections b->sec marks derived, behind the copies on st
int ald_set_err(int code, const std::string &msg);        // sets the calling thread's ald_last_error() text, returns `code`
