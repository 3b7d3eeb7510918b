// tset_index.hip -- the transcript boundaries of a stream that lies in device memory, found without the host's record walk.
//
// A transcript stream (format of ald_batch_transcript_stream) has no index: record i + 1 begins where record i ends, and a record's length
// is in its own header (ts_words: ALD_TS_HDR + 2 * n_exons).  The host walks it record by record (tx_stream_records).  But "the next record" is a
// function EVERY word position can evaluate by itself, and the real boundaries are what that function reaches from position 0: list
// ranking.  Lengths are even, so only even positions are candidates; position o = 2 h is node h, and two extra nodes that point to
// themselves end every chain: END (= n_words, the stream is consumed exactly) and BAD (a header that does not fit, a negative count, a
// record that overruns).  A payload whose words happen to read as headers makes chains of its own -- they may even merge into the true one
// or end on END -- but nothing is marked that position 0 does not reach.
//
// Kernels (streaming passes over n_words / 2 nodes; select and scan are hipCUB):
//   ix_succ     1 lane / node        successor in 64-bit arithmetic, never reading past n_words; mark = {node 0}
//   ix_jump     1 lane / node        one round of pointer doubling: a marked node marks its successor, then succ <- succ o succ, read from
//                                    the previous round's buffer and written to the other.  After round k everything within 2^k - 1 links
//                                    of position 0 is marked; a chain has at most n_words / ALD_TS_HDR + 1 links, which fixes the number of rounds.
//                                    (A mark set in this round and seen by another lane of the same round only marks a node early that a
//                                    later round would mark anyway: marks only ever go to nodes position 0 reaches.)
//   select      hipCUB               marked positions in ascending order: toff[0 .. nt)
//   ix_graphs   1 lane / transcript  graph id (unsigned, as the host walk widens it), head of a run of equal ids, descending pair -> flag
//   scan        hipCUB               inclusive sum of the heads: 1-based group of every transcript (counted BEFORE any single-exon filter)
//   ix_labels   1 lane / transcript  label[group] = graph id + graph_offset, sid[group] = ALD_TS_SID of the run's first transcript; the counts
//                                    and the flags into one small block that goes to the host in a single copy
#include "tset_front.h"
#include <hipcub/hipcub.hpp>

namespace {

__device__ inline int64_t ix_lane() { return (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x; }

// nodes 0 .. M - 1: the even positions below n_words; M: END (a successor n_words is node n_words / 2 = M; with an odd n_words no
// even successor equals it and END stays unreached); M + 1: BAD
__global__ void ix_succ(const uint32_t *words, int64_t n_words, uint32_t M, uint32_t *succ, uint8_t *mark)
{
    const int64_t i = ix_lane();
    if(i >= (int64_t)M + 2) return;
    uint32_t nx = (uint32_t)i;                               // END and BAD point to themselves
    if(i < (int64_t)M) {
        const int64_t o = 2 * i; nx = M + 1;
        if(o + ALD_TS_HDR <= n_words) {
            const uint32_t *w = words + o;
            const int64_t t = o + ts_words(w);
            if((int32_t)w[ALD_TS_NEXONS] >= 0 && t <= n_words) nx = (uint32_t)(t >> 1);
        }
    }
    succ[i] = nx; mark[i] = i == 0 ? 1 : 0;
}
__global__ void ix_jump(const uint32_t *succ, uint32_t *next, uint8_t *mark, uint32_t n_nodes)
{
    const int64_t i = ix_lane();
    if(i >= (int64_t)n_nodes) return;
    const uint32_t a = succ[i];
    if(mark[i]) mark[a] = 1;
    next[i] = succ[a];
}
struct IxTwice { __host__ __device__ unsigned long long operator()(unsigned long long h) const { return 2 * h; } };

// sum: [0] nt (written by the select), [1] groups, [2] END reached, [3] BAD reached, [4] a descending pair (zeroed before the launch)
__global__ void ix_graphs(const uint32_t *words, int64_t n_words, unsigned long long *toff, int64_t cap, unsigned long long *sum, int32_t *head)
{
    const int64_t i = ix_lane();
    if(i >= cap) return;
    const int64_t nt = (int64_t)sum[0];
    if(i == 0) toff[nt] = (unsigned long long)n_words;
    if(i >= nt) { head[i] = 0; return; }                     // (the scan runs over all `cap` entries: no count has to reach the host first)
    const uint32_t g = words[toff[i] + ALD_TS_GRAPH];
    if(i == 0) { head[i] = 1; return; }
    const uint32_t pg = words[toff[i - 1] + ALD_TS_GRAPH];
    head[i] = g != pg ? 1 : 0;
    if(g < pg) sum[4] = 1;
}
__global__ void ix_labels(const uint32_t *words, int64_t n_words, const unsigned long long *toff, int64_t cap, const int32_t *head, const int32_t *gid, const uint8_t *mark, uint32_t M,
                          int64_t graph_offset, unsigned long long *sum, int64_t *label, int32_t *sid)
{
    const int64_t i = ix_lane();
    if(i >= cap) return;
    const int64_t nt = (int64_t)sum[0];
    if(i == 0) { sum[1] = nt > 0 ? (unsigned long long)gid[nt - 1] : 0; sum[2] = mark[M]; sum[3] = mark[M + 1]; }
    if(i >= nt || !head[i]) return;
    const int64_t o = (int64_t)toff[i]; const int32_t k = gid[i] - 1;
    label[k] = (int64_t)words[o + ALD_TS_GRAPH] + graph_offset;
    sid[k] = o + ALD_TS_SID < n_words ? (int32_t)words[o + ALD_TS_SID] : 0;   // (only the last marked position of a malformed stream can lie this close to the end)
}

} // namespace

int tx_stream_index(hipStream_t st, StreamIndexScratch &X, hipEvent_t e0, hipEvent_t e1, const uint32_t *d_words, int64_t n_words, int64_t graph_offset, StreamIndex &I)
{
    I = StreamIndex();
    if(n_words <= 0) return ALD_OK;
    if(n_words >= (int64_t)1 << 31) return ald_set_err(ALD_ERR_INVALID, "stream index: 2^31 words or more");
    const uint32_t M = (uint32_t)((n_words + 1) / 2); const int64_t N = (int64_t)M + 2, cap = n_words / ALD_TS_HDR + 1;
    DevBuf &d_a = X.succ, &d_b = X.succ_next, &d_mark = X.mark, &d_toff = X.toff, &d_head = X.head, &d_gid = X.gid, &d_label = X.label, &d_sid = X.sid, &d_tmp = X.cub_tmp, &d_sum = X.sum;
    PinBuf &pin = X.p_sum;
    if(d_a.ensure(4 * (size_t)N) || d_b.ensure(4 * (size_t)N) || d_mark.ensure((size_t)N) || d_toff.ensure(8 * (size_t)(cap + 1)) || d_head.ensure(4 * (size_t)cap) || d_gid.ensure(4 * (size_t)cap)
       || d_label.ensure(8 * (size_t)cap) || d_sid.ensure(4 * (size_t)cap) || d_sum.ensure(64) || pin.ensure(64)) return ald_set_err(ALD_ERR_NOMEM, "stream index buffers");
    hipcub::CountingInputIterator<unsigned long long> count(0);
    hipcub::TransformInputIterator<unsigned long long, IxTwice, hipcub::CountingInputIterator<unsigned long long>> pos(count, IxTwice());
    unsigned long long *sum = (unsigned long long*)d_sum.p;
    int rounds = 0; while(((int64_t)1 << rounds) <= cap) rounds++;          // 2^rounds - 1 >= cap = the most links a chain can have
    if(e0) HCHK(hipEventRecord(e0, st));
    HCHK(hipMemsetAsync(d_sum.p, 0, 64, st));
    hipLaunchKernelGGL(ix_succ, dim3(grid_for(N)), dim3(TX_BLOCK), 0, st, d_words, n_words, M, (uint32_t*)d_a.p, (uint8_t*)d_mark.p);
    uint32_t *cur = (uint32_t*)d_a.p, *nxt = (uint32_t*)d_b.p;
    for(int r = 0; r < rounds; r++) { hipLaunchKernelGGL(ix_jump, dim3(grid_for(N)), dim3(TX_BLOCK), 0, st, (const uint32_t*)cur, nxt, (uint8_t*)d_mark.p, (uint32_t)N); std::swap(cur, nxt); }
    { int rc = tx_cub(d_tmp, "stream index scratch", [&](void *t, size_t &nb) { return hipcub::DeviceSelect::Flagged(t, nb, pos, (const uint8_t*)d_mark.p, (unsigned long long*)d_toff.p, sum, (int)M, st); }); if(rc != ALD_OK) return rc; }
    hipLaunchKernelGGL(ix_graphs, dim3(grid_for(cap)), dim3(TX_BLOCK), 0, st, d_words, n_words, (unsigned long long*)d_toff.p, cap, sum, (int32_t*)d_head.p);
    { int rc = tx_cub(d_tmp, "stream index scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::InclusiveSum(t, nb, (const int32_t*)d_head.p, (int32_t*)d_gid.p, (int)cap, st); }); if(rc != ALD_OK) return rc; }
    hipLaunchKernelGGL(ix_labels, dim3(grid_for(cap)), dim3(TX_BLOCK), 0, st, d_words, n_words, (const unsigned long long*)d_toff.p, cap, (const int32_t*)d_head.p, (const int32_t*)d_gid.p,
                       (const uint8_t*)d_mark.p, M, graph_offset, sum, (int64_t*)d_label.p, (int32_t*)d_sid.p);
    if(e1) HCHK(hipEventRecord(e1, st));
    HCHK(hipMemcpyAsync(pin.p, d_sum.p, 40, hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a stream-index kernel failed to launch");
    const unsigned long long *h = (const unsigned long long*)pin.p;
    I.toff = (const unsigned long long*)d_toff.p; I.gid = (const int32_t*)d_gid.p; I.label = (const int64_t*)d_label.p; I.sid = (const int32_t*)d_sid.p;
    I.nt = (int64_t)h[0]; I.ng = (int64_t)h[1];
    if(e0 && e1) { float ms = 0; if(hipEventElapsedTime(&ms, e0, e1) == hipSuccess) I.ms = ms; }
    if(!h[2] || h[3]) return ald_set_err(ALD_ERR_INVALID, "malformed transcript stream");
    if(h[4]) return ald_set_err(ALD_ERR_INVALID, "transcript stream not in ascending graph order");
    return ALD_OK;
}

extern "C" {

int ald_tset_index_stream(int32_t device, const uint32_t *words, int64_t n_words, int64_t *offsets, int64_t capacity, int64_t *n_transcripts, int64_t *n_graphs)
{
    if(n_words < 0 || (n_words > 0 && !words) || (offsets && capacity < 0)) return ALD_ERR_INVALID;
    { int rc = tx_need_device(device, "the stream index"); if(rc != ALD_OK) return rc; }
    HCHK(hipSetDevice(device));
    if(n_transcripts) *n_transcripts = 0; if(n_graphs) *n_graphs = 0;
    const bool src_dev = tx_on_device(words), dst_dev = tx_on_device(offsets);
    const int64_t zero = 0;
    if(n_words == 0) {
        if(offsets && capacity < 1) return ald_set_err(ALD_ERR_INVALID, "stream index: offsets too small");
        if(offsets) { if(dst_dev) HCHK(hipMemcpy(offsets, &zero, 8, hipMemcpyHostToDevice)); else offsets[0] = 0; }
        return ALD_OK;
    }
    Scoped<StreamIndexScratch> ix; Scoped<DevBuf> d_in;
    ScopedStream stream; HCHK(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    hipStream_t st = stream.s;
    if(n_words >= (int64_t)1 << 31) return ald_set_err(ALD_ERR_INVALID, "stream index: 2^31 words or more");
    if(!src_dev) { if(d_in.ensure(4 * (size_t)n_words)) return ald_set_err(ALD_ERR_NOMEM, "stream index buffers"); HCHK(hipMemcpyAsync(d_in.p, words, 4 * (size_t)n_words, hipMemcpyHostToDevice, st)); }
    StreamIndex I;
    const int rc = tx_stream_index(st, ix, nullptr, nullptr, src_dev ? words : (const uint32_t*)d_in.p, n_words, 0, I);
    if(rc != ALD_OK) return rc;
    if(n_transcripts) *n_transcripts = I.nt; if(n_graphs) *n_graphs = I.ng;
    if(offsets) {
        if(capacity < I.nt + 1) return ald_set_err(ALD_ERR_INVALID, "stream index: offsets too small");
        HCHK(hipMemcpy(offsets, I.toff, 8 * (size_t)(I.nt + 1), dst_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    }
    return ALD_OK;
}

} // extern "C"
