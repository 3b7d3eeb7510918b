// tset_reduce.hip -- transcript-set reduction of a whole batch on the GPU.
//
// What it replaces: the loop of assembler::assemble over the graphs of one region (meta/assembler.cc:1105-1133) -- per graph a local
// transcript_set `ts` filled by ts.add(t, 1, sid) (rnacore/transcript_set.cc:149-154), then tm.add(ts) (:156-175) into the region's
// set -- i.e. bucketing by intron-chain hash (gtf/transcript.cc:183-201), ordering / equality by compare1 (:269-300) and
// trans_item::merge (transcript_set.cc:38-81), for the case the reference runs it in: a set that starts EMPTY and takes the graphs in
// ascending order.  (Merging two finished sets is a separate, cheap step: ald_tset_add_flat below = transcript_set::add(set).)
//
// Why it splits the way it does.  For transcripts with two or more exons compare1 is a plain lexicographic order on (number of
// exons, strand, the compared coordinates), so "equal" is an equivalence relation and everything a merge computes is independent of
// the order of the merges -- counts add, cov2 / conf / abd / count1 and the per-sample copies take maxima, the outer bounds widen --
// except ONE thing: the floating-point sum of the coverages, which the reference forms as  ((s1 + s2) + s3) + ...  over the graphs
// that contribute, s_k itself being the left-to-right sum inside graph k.  So: sort the transcripts by group (stable, they start in
// (graph, path) order), and let one lane per group fold its members in exactly that nesting.  Single-exon transcripts merge by an
// overlap test that is not transitive (transcript.cc:283-291): their result depends on the sequence of comparisons, they are few,
// and they go through the host sink (aletsch_amd/host/transcript_sink.hpp) as before.
//
// Kernels (HBM-bound streaming passes over ~2 M transcripts of ~80 B; the sorts are hipCUB radix sorts):
//   tx_build      1 lane / path     record -> joined exons (essential.cc:735-746) -> bucket hash, group key
//   tx_heads      1 lane / sorted   first member of a group?  (keys equal AND the compared words equal: a key collision splits, never fuses)
//   tx_fold       1 lane / group    coverage in the reference's nesting, count, maxima, bounds
//   tx_skeys / tx_sheads / tx_sfold    the per-sample copies: (group, sample) runs after a second stable sort, maxima per run
#include "tset_front.h"
#include <hipcub/hipcub.hpp>
#include <cmath>
#include <thread>
#include <memory>
#include <chrono>

namespace {

// ---- the result index in (graph, path) order: prefix of the per-graph path counts, then one lane per graph copies its entries
__global__ void ix_order(const int32_t *n_paths, const int64_t *pbegin, const long long *graph_first, const unsigned long long *index, int n, unsigned long long *ordoff)
{
    const int g = (int)((int64_t)blockIdx.x * TX_BLOCK + threadIdx.x);
    if(g >= n) return;
    const int c = n_paths[g]; const long long f = graph_first[g]; const int64_t o = pbegin[g];
    if(f < 0) return;
    for(int p = 0; p < c; p++) ordoff[o + p] = index[f + p];
}
__global__ void ix_widen(const int32_t *n_paths, int n, int64_t *len) { const int g = (int)((int64_t)blockIdx.x * TX_BLOCK + threadIdx.x); if(g <= n) len[g] = g < n ? (int64_t)n_paths[g] : 0; }

// WEIGHT: also weight[p] = the record's weight (ALD_REC_WEIGHT), dense in (graph, path) order -- consecutive lanes write consecutive doubles -- for a
// caller that has no host copy of the records and takes coverage = log(1 + weight) on the host (tx_front_coverage)
template<bool WEIGHT> __global__ void tx_build(TxIn in, int32_t *nwords, uint64_t *key, int32_t *graph_of, double *weight)
{
    const int64_t p = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(p >= in.np) return;
    const uint32_t *r = in.pool + in.roff[p];
    const int g = (int)r[ALD_REC_GRAPH], k = (int)r[ALD_REC_NEXW]; const int strand = (int)rec_strand(r);
    const int32_t *ex = rec_exons(r);
    nwords[p] = k; graph_of[p] = g;
    if(WEIGHT) { double w; memcpy(&w, r + ALD_REC_WEIGHT, 8); weight[p] = w; }
    if(k <= 2) { key[p] = TX_HOST; return; }
    const uint64_t bucket = chain_key_dev(ex, k);
    // group = (bucket, exons, strand, the words compare1 looks at: 1, 2 .. k-5, k-2); 32 bits of it ride in the sort key
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h ^= v; h *= 1099511628211ull; h ^= h >> 29; };
    mix((uint64_t)k); mix((uint64_t)strand); mix((uint64_t)(uint32_t)ex[1]);
    for(int q = 2; q + 5 <= k; q++) mix((uint64_t)(uint32_t)ex[q]);
    mix((uint64_t)(uint32_t)ex[k - 2]);
    uint64_t kk = (bucket << 32) | (h & 0xFFFFFFFFull);
    if(kk == TX_HOST) kk--;
    key[p] = kk;
}

// same group as the previous sorted element?  equal key AND equal (exon count, strand, compared words, bucket)
__device__ inline bool same_group(const TxIn &in, int64_t a, int64_t b)
{
    const uint32_t *ra = in.pool + in.roff[a], *rb = in.pool + in.roff[b];
    const int ka = (int)ra[ALD_REC_NEXW], kb = (int)rb[ALD_REC_NEXW];
    if(ka != kb) return false;
    if(rec_strand(ra) != rec_strand(rb)) return false;
    const int32_t *xa = rec_exons(ra), *xb = rec_exons(rb);
    if(xa[1] != xb[1] || xa[ka - 2] != xb[ka - 2]) return false;
    for(int q = 2; q + 5 <= ka; q++) if(xa[q] != xb[q]) return false;
    return chain_key_dev(xa, ka) == chain_key_dev(xb, kb);
}

__global__ void tx_heads(TxIn in, const uint64_t *skey, const int64_t *sidx, int64_t n_dev, int32_t *head)
{
    const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(i >= n_dev) return;
    head[i] = (i == 0 || skey[i] != skey[i - 1] || !same_group(in, sidx[i - 1], sidx[i])) ? 1 : 0;
}

// start_idx / start_cov (null for a set that starts empty): the resident item a group lands on -- its coverage is where the sum starts
__global__ void tx_fold(TxIn in, const uint64_t *skey, const int64_t *sidx, const int32_t *head, const int32_t *gid, int64_t n_dev, const double *cov,
                        const int64_t *start_idx, const double *start_cov, TxGroup *out)
{
    const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(i >= n_dev || !head[i]) return;
    TxGroup G; G.first = sidx[i]; G.first_off = in.roff[sidx[i]]; G.bucket = (uint32_t)(skey[i] >> 32); G.count = 0; G.count1 = 0; G.coverage = 0; G.cov2 = 0; G.conf = 0; G.abd = 0; G.lo = 0; G.hi = 0; G.pad = 0;
    { const uint32_t *r0 = in.pool + G.first_off; G.nw = (int32_t)r0[ALD_REC_NEXW]; G.graph = (int32_t)r0[ALD_REC_GRAPH]; G.path = (int32_t)r0[ALD_REC_PATH]; G.strand = (int32_t)rec_strand(r0); }
    double inner = 0; int cur_g = -1; bool any = false;
    if(start_idx) { const int64_t z = start_idx[gid[i] - 1]; if(z >= 0) { G.coverage = start_cov[z]; any = true; } }
    for(int64_t m = i; m < n_dev && (m == i || !head[m]); m++) {
        const int64_t p = sidx[m]; const uint32_t *r = in.pool + in.roff[p];
        const int g = (int)r[ALD_REC_GRAPH]; const double c = cov[p];
        double conf, abd; memcpy(&abd, r + ALD_REC_ABD, 8); memcpy(&conf, r + ALD_REC_CONF, 8);
        const int32_t *x = rec_exons(r); const int k = (int)r[ALD_REC_NEXW];
        if(g != cur_g) {                                 // the previous graph's own sum enters the set: moved in if the set had none, else added
            if(cur_g >= 0) { G.coverage = any ? G.coverage + inner : inner; any = true; }
            inner = c; cur_g = g;
        } else inner += c;                               // trans_item::merge inside the graph's own set (coverage adds for >= 2 exons)
        if(m == i) { G.lo = x[0]; G.hi = x[k - 1]; G.cov2 = c; G.conf = conf; G.abd = abd; G.count1 = (int32_t)r[ALD_REC_COUNT]; }
        else {
            if(x[0] < G.lo) G.lo = x[0]; if(x[k - 1] > G.hi) G.hi = x[k - 1];
            if(G.cov2 < c) G.cov2 = c; if(G.conf < conf) G.conf = conf; if(G.abd < abd) G.abd = abd; if(G.count1 < (int32_t)r[ALD_REC_COUNT]) G.count1 = (int32_t)r[ALD_REC_COUNT];
        }
        G.count++;
    }
    G.coverage = any ? G.coverage + inner : inner;
    out[gid[i] - 1] = G;                                  // gid: inclusive scan of the head flags, 1-based
}

__global__ void tx_skeys(const int64_t *sidx, const int32_t *gid_incl, const int32_t *graph_of, const int32_t *sid, int64_t n_dev, uint64_t *key2)
{
    const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(i >= n_dev) return;
    const int s = sid ? sid[graph_of[sidx[i]]] : -1;
    key2[i] = ((uint64_t)(uint32_t)gid_incl[i] << 32) | (uint64_t)(uint32_t)(s + 1);      // sample ids ascend as the reference's std::map does (-1 first)
}
__global__ void tx_sheads(const uint64_t *skey2, int64_t n_dev, int32_t *head2)
{
    const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(i >= n_dev) return;
    head2[i] = (i == 0 || skey2[i] != skey2[i - 1]) ? 1 : 0;
}
__global__ void tx_sfold(TxIn in, const uint64_t *skey2, const int64_t *spos, const int64_t *sidx, const int32_t *head2, const int32_t *rid, int64_t n_dev, const double *cov, TxSample *out)
{
    const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(i >= n_dev || !head2[i]) return;
    TxSample S; S.gid = (int32_t)(skey2[i] >> 32) - 1; S.sid = (int32_t)(uint32_t)(skey2[i] & 0xFFFFFFFFull) - 1; S.count1 = 0; S.pad = 0; S.cov2 = 0; S.conf = 0; S.abd = 0;
    for(int64_t m = i; m < n_dev && (m == i || !head2[m]); m++) {
        const int64_t p = sidx[spos[m]]; const uint32_t *r = in.pool + in.roff[p];
        double conf, abd; memcpy(&abd, r + ALD_REC_ABD, 8); memcpy(&conf, r + ALD_REC_CONF, 8); const double c = cov[p];
        if(m == i) { S.cov2 = c; S.conf = conf; S.abd = abd; S.count1 = (int32_t)r[ALD_REC_COUNT]; }
        else { if(S.cov2 < c) S.cov2 = c; if(S.conf < conf) S.conf = conf; if(S.abd < abd) S.abd = abd; if(S.count1 < (int32_t)r[ALD_REC_COUNT]) S.count1 = (int32_t)r[ALD_REC_COUNT]; }
    }
    out[rid[i] - 1] = S;
}
__global__ void tx_iota(int64_t *v, int64_t n) { const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x; if(i < n) v[i] = i; }

// ---- the finished transcripts of a batch as one stream IN DEVICE MEMORY (ald_batch_device_transcript_stream): what ranks exchange
__global__ void ts_len(TxIn in, int skip_single, int64_t *len)
{
    const int64_t p = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(p > in.np) return;
    if(p == in.np) { len[p] = 0; return; }                // (the exclusive scan over np + 1 entries leaves the total in the last one)
    const int k = (int)in.pool[in.roff[p] + ALD_REC_NEXW];
    len[p] = (k <= 2 && skip_single) ? 0 : (int64_t)ALD_TS_HDR + k;
}
// one 16-lane group per transcript: header by the first lanes, exon words copied with consecutive lanes on consecutive words
__global__ void ts_emit(TxIn in, const int64_t *at, const int32_t *sid, uint32_t *out)
{
    const int64_t p = ((int64_t)blockIdx.x * TX_BLOCK + threadIdx.x) / 16; const int l = (int)(threadIdx.x & 15);
    if(p >= in.np) return;
    const int64_t o = at[p];
    if(at[p + 1] == o) return;
    const uint32_t *r = in.pool + in.roff[p]; const int k = (int)r[ALD_REC_NEXW];
    uint32_t *w = out + o;
    if(l < ALD_TS_HDR) w[l] = ts_header_word(r, l, sid);
    const uint32_t *x = (const uint32_t*)rec_exons(r);
    for(int q = l; q < k; q += 16) w[ALD_TS_HDR + q] = x[q];
}

// ---- the records of the transcripts the host merges (fewer than two exons), compacted: hp[a] = path of the a-th of them
__global__ void sx_len(TxIn in, const int64_t *hp, int64_t ns, int64_t *len)
{
    const int64_t a = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(a > ns) return;
    if(a == ns) { len[a] = 0; return; }                   // (the exclusive scan over ns + 1 entries leaves the total in the last one)
    const uint32_t *r = in.pool + in.roff[hp[a]];
    len[a] = (int64_t)rec_words(r[ALD_REC_NV], r[ALD_REC_NEXW]);       // header + vertices + exon words, padded to even
}
// one 16-lane group per record, consecutive lanes on consecutive words (as ts_emit copies)
__global__ void sx_copy(TxIn in, const int64_t *hp, const int64_t *at, int64_t ns, uint32_t *out)
{
    const int64_t a = ((int64_t)blockIdx.x * TX_BLOCK + threadIdx.x) / 16; const int l = (int)(threadIdx.x & 15);
    if(a >= ns) return;
    const uint32_t *r = in.pool + in.roff[hp[a]];
    const int64_t o = at[a], w = at[a + 1] - o;
    for(int64_t q = l; q < w; q += 16) out[o + q] = r[q];
}

} // namespace

// The result index of a downloaded or finished batch in (graph, path) order, in DEVICE memory: d_ordoff[path_begin[g] + p] = pool offset of record
// (g, p).  Everything comes from what the decomposition kernel left in HBM -- the per-graph path counts, graph_first and the index
// entries -- so the transcript stream and the set reduction start without any host-side table.
int device_path_table(ald_batch *b)
{
    if(b->paths_on_device) return ALD_OK;
    const int n = b->hb.n(); const int64_t np = b->total_paths;
    if(n == 0 || np == 0) { b->paths_on_device = true; return ALD_OK; }
    DevBuf &d_len = b->d_ts_len;
    if(b->d_pbegin.ensure(8 * (size_t)n + 8) || b->d_ordoff.ensure(8 * (size_t)np + 8) || d_len.ensure(8 * (size_t)n + 8)) return ald_set_err(ALD_ERR_NOMEM, "device path table");
    hipStream_t st = b->stream;
    hipLaunchKernelGGL(ix_widen, dim3(grid_for(n + 1)), dim3(TX_BLOCK), 0, st, (const int32_t*)b->d_npaths.p, n, (int64_t*)d_len.p);
    { int rc = tx_cub(b->tx.cub_tmp, "scan scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int64_t*)d_len.p, (int64_t*)b->d_pbegin.p, n + 1, st); }); if(rc != ALD_OK) return rc; }
    hipLaunchKernelGGL(ix_order, dim3(grid_for(n)), dim3(TX_BLOCK), 0, st, (const int32_t*)b->d_npaths.p, (const int64_t*)b->d_pbegin.p, (const long long*)b->d_gfirst.p, (const unsigned long long*)b->d_index.p, n, (unsigned long long*)b->d_ordoff.p);
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a path-table kernel failed to launch");
    b->paths_on_device = true;
    return ALD_OK;
}

int tx_front_sort(RedScratch S, TxIn in, const double *h_cov, int n_graphs, const int32_t *sid, TxFront &F)
{
    const int64_t np = in.np;
    F.np = np; F.n_dev = 0; F.n_groups = 0; F.n_runs = 0; F.host_paths.clear(); F.sid_on_device = sid != nullptr; F.h_cov = nullptr;
    if(np == 0) { if(F.ev0) HCHK(hipEventRecord(F.ev0, S.st)); return ALD_OK; }
    TxScratch &X = *S.x;
    DevBuf &d_cov = X.cov, &d_w = X.weight, &d_nw = X.nw, &d_key = X.key, &d_key2 = X.key_sorted, &d_idx = X.idx, &d_idx2 = X.sidx, &d_graph = X.graph,
           &d_sid = X.sid, &d_head = X.head, &d_gid = X.gid, &d_head2 = X.run_head, &d_rid = X.run_id, &d_pos = X.pos, &d_pos2 = X.pos_sorted;
    PinBuf &p_key = X.p_key, &p_w = X.p_weight, &p_cov = X.p_cov;
    const bool from_records = h_cov == nullptr && F.d_cov == nullptr;
    if(from_records && !F.ev_w) return ald_set_err(ALD_ERR_INVALID, "tx_front_sort: coverage from the records needs an event");
    if(p_key.ensure(8 * (size_t)np, true) || (from_records && (p_w.ensure(8 * (size_t)np, true) || p_cov.ensure(8 * (size_t)np)))) return ald_set_err(ALD_ERR_NOMEM, "pinned reduction buffers");
    if(d_cov.ensure(8 * (size_t)np) || d_nw.ensure(4 * (size_t)np) || d_key.ensure(8 * (size_t)np) || (from_records && d_w.ensure(8 * (size_t)np))
       || d_key2.ensure(8 * (size_t)np) || d_idx.ensure(8 * (size_t)np) || d_idx2.ensure(8 * (size_t)np) || d_graph.ensure(4 * (size_t)np) || d_head.ensure(4 * (size_t)np) || d_gid.ensure(4 * (size_t)np)
       || d_head2.ensure(4 * (size_t)np) || d_rid.ensure(4 * (size_t)np) || d_pos.ensure(8 * (size_t)np) || d_pos2.ensure(8 * (size_t)np) || (sid && d_sid.ensure(4 * (size_t)n_graphs + 4))) return ald_set_err(ALD_ERR_NOMEM, "reduction buffers");
    hipStream_t st = S.st;
    if(h_cov) HCHK(hipMemcpyAsync(d_cov.p, h_cov, 8 * (size_t)np, hipMemcpyHostToDevice, st));
    else if(F.d_cov) HCHK(hipMemcpyAsync(d_cov.p, F.d_cov, 8 * (size_t)np, hipMemcpyDeviceToDevice, st));
    if(sid) HCHK(hipMemcpyAsync(d_sid.p, sid, 4 * (size_t)n_graphs, hipMemcpyHostToDevice, st));
    if(F.ev0) HCHK(hipEventRecord(F.ev0, st));
    if(from_records) {
        hipLaunchKernelGGL(tx_build<true>, dim3(grid_for(np)), dim3(TX_BLOCK), 0, st, in, (int32_t*)d_nw.p, (uint64_t*)d_key.p, (int32_t*)d_graph.p, (double*)d_w.p);
        HCHK(hipMemcpyAsync(p_w.p, d_w.p, 8 * (size_t)np, hipMemcpyDeviceToHost, st)); tx_count_d2h(S, 8 * (size_t)np);
        HCHK(hipEventRecord(F.ev_w, st));
    } else hipLaunchKernelGGL(tx_build<false>, dim3(grid_for(np)), dim3(TX_BLOCK), 0, st, in, (int32_t*)d_nw.p, (uint64_t*)d_key.p, (int32_t*)d_graph.p, (double*)nullptr);
    hipLaunchKernelGGL(tx_iota, dim3(grid_for(np)), dim3(TX_BLOCK), 0, st, (int64_t*)d_idx.p, np);
    // stable sort by group key: members of a group stay in (graph, path) order; host-side transcripts (key = ~0) sink to the end
    { int rc = tx_cub(X.cub_tmp, "sort scratch", [&](void *t, size_t &nb) { return hipcub::DeviceRadixSort::SortPairs(t, nb, (const uint64_t*)d_key.p, (uint64_t*)d_key2.p, (const int64_t*)d_idx.p, (int64_t*)d_idx2.p, (int)np, 0, 64, st); }); if(rc != ALD_OK) return rc; }
    // how many went to the device: the sorted keys below TX_HOST (tx_front_heads looks)
    HCHK(hipMemcpyAsync(p_key.p, d_key2.p, 8 * (size_t)np, hipMemcpyDeviceToHost, st)); tx_count_d2h(S, 8 * (size_t)np);
    return ALD_OK;
}

int tx_front_coverage(RedScratch S, TxFront &F)
{
    const int64_t np = F.np;
    if(np == 0) return ALD_OK;
    HCHK(hipEventSynchronize(F.ev_w));                     // the weights are in pinned memory; the sort is running
    const double *w = (const double*)S.x->p_weight.p; double *cov = (double*)S.x->p_cov.p;
    const unsigned nthr = ald_sink_threads(np);
    HostBatch::run_threads(nthr, [&](unsigned th) { for(int64_t i = np * th / nthr; i < np * (th + 1) / nthr; i++) cov[(size_t)i] = log(1.0 + w[(size_t)i]); });      // essential.cc:725, host libm
    HCHK(hipMemcpyAsync(S.x->cov.p, cov, 8 * (size_t)np, hipMemcpyHostToDevice, S.st));
    F.h_cov = cov;
    return ALD_OK;
}

int tx_front_heads(RedScratch S, TxIn in, TxFront &F)
{
    const int64_t np = F.np;
    if(np == 0) return ALD_OK;
    DevBuf &d_key2 = S.x->key_sorted, &d_idx2 = S.x->sidx, &d_head = S.x->head, &d_gid = S.x->gid;
    hipStream_t st = S.st;
    const uint64_t *h_key = (const uint64_t*)S.x->p_key.p;
    HCHK(hipStreamSynchronize(st));
    const int64_t n_dev = (int64_t)(std::lower_bound(h_key, h_key + np, TX_HOST) - h_key);
    F.n_dev = n_dev;
    if(n_dev > 0) {
        hipLaunchKernelGGL(tx_heads, dim3(grid_for(n_dev)), dim3(TX_BLOCK), 0, st, in, (const uint64_t*)d_key2.p, (const int64_t*)d_idx2.p, n_dev, (int32_t*)d_head.p);
        { int rc = tx_cub(S.x->cub_tmp, "scan scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::InclusiveSum(t, nb, (const int32_t*)d_head.p, (int32_t*)d_gid.p, (int)n_dev, st); }); if(rc != ALD_OK) return rc; }
        HCHK(hipMemcpyAsync(&F.n_groups, (int32_t*)d_gid.p + (n_dev - 1), 4, hipMemcpyDeviceToHost, st)); tx_count_d2h(S, 4);
    }
    // the transcripts left to the host: the tail of the sorted order (key TX_HOST; the stable sort kept them in (graph, path) order)
    F.host_paths.resize((size_t)(np - n_dev));
    if(np > n_dev) { HCHK(hipMemcpyAsync(F.host_paths.data(), (const int64_t*)d_idx2.p + n_dev, 8 * (size_t)(np - n_dev), hipMemcpyDeviceToHost, st)); tx_count_d2h(S, 8 * (size_t)(np - n_dev)); }
    HCHK(hipStreamSynchronize(st));
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a reduction kernel failed to launch");
    return ALD_OK;
}

int tx_front_groups(RedScratch S, TxIn in, const double *h_cov, int n_graphs, const int32_t *sid, TxFront &F)
{
    if(!h_cov && in.np > 0) return ald_set_err(ALD_ERR_INVALID, "tx_front_groups: no coverages");
    { int rc = tx_front_sort(S, in, h_cov, n_graphs, sid, F); if(rc != ALD_OK) return rc; }
    return tx_front_heads(S, in, F);
}

int tx_compact_singles(RedScratch S, TxIn in, const TxFront &F, DevBuf &d_out, const uint32_t **h_words, const unsigned long long **h_off)
{
    const int64_t ns = (int64_t)F.host_paths.size();
    *h_words = nullptr; *h_off = nullptr;
    if(ns == 0) return ALD_OK;
    DevBuf &d_len = S.x->single_len, &d_at = S.x->single_at;
    PinBuf &p_off = S.x->p_single_off, &p_words = S.x->p_single_words;
    hipStream_t st = S.st;
    const int64_t *hp = tx_sidx(S) + F.n_dev;             // the tail of the sorted order, still on the device
    if(d_len.ensure(8 * (size_t)(ns + 1)) || d_at.ensure(8 * (size_t)(ns + 1)) || p_off.ensure(8 * (size_t)(ns + 1), true)) return ald_set_err(ALD_ERR_NOMEM, "single-exon compaction");
    hipLaunchKernelGGL(sx_len, dim3(grid_for(ns + 1)), dim3(TX_BLOCK), 0, st, in, hp, ns, (int64_t*)d_len.p);
    { int rc = tx_cub(S.x->cub_tmp, "scan scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int64_t*)d_len.p, (int64_t*)d_at.p, (int)(ns + 1), st); }); if(rc != ALD_OK) return rc; }
    HCHK(hipMemcpyAsync(p_off.p, d_at.p, 8 * (size_t)(ns + 1), hipMemcpyDeviceToHost, st)); tx_count_d2h(S, 8 * (size_t)(ns + 1));
    HCHK(hipStreamSynchronize(st));
    const int64_t total = ((const int64_t*)p_off.p)[ns];
    if(total < 0 || d_out.ensure(4 * (size_t)total + 64) || p_words.ensure(4 * (size_t)total + 64, true)) return ald_set_err(ALD_ERR_NOMEM, "single-exon records");
    hipLaunchKernelGGL(sx_copy, dim3(grid_for(16 * ns)), dim3(TX_BLOCK), 0, st, in, hp, (const int64_t*)d_at.p, ns, (uint32_t*)d_out.p);
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a compaction kernel failed to launch");
    if(total) { HCHK(hipMemcpyAsync(p_words.p, d_out.p, 4 * (size_t)total, hipMemcpyDeviceToHost, st)); tx_count_d2h(S, 4 * (size_t)total); }
    *h_words = (const uint32_t*)p_words.p; *h_off = (const unsigned long long*)p_off.p;
    return ALD_OK;
}

int tx_front_fold(RedScratch S, TxIn in, TxFront &F, const int64_t *start_idx, const double *start_cov)
{
    const int64_t n_dev = F.n_dev; F.n_runs = 0;
    if(n_dev == 0) return ALD_OK;
    TxScratch &X = *S.x;
    DevBuf &d_cov = X.cov, &d_graph = X.graph, &d_sid = X.sid, &d_groups = X.groups, &d_head2 = X.run_head, &d_rid = X.run_id, &d_samples = X.samples, &d_pos = X.pos, &d_pos2 = X.pos_sorted;
    DevBuf &d_skey = X.key, &d_skey2 = X.idx;                // second lives: both are free once the first sort is done and its keys are in key_sorted
    hipStream_t st = S.st;
    const uint64_t *skey = tx_skey(S); const int64_t *sidx = tx_sidx(S);
    if(d_groups.ensure(sizeof(TxGroup) * (size_t)F.n_groups)) return ald_set_err(ALD_ERR_NOMEM, "group records");
    hipLaunchKernelGGL(tx_fold, dim3(grid_for(n_dev)), dim3(TX_BLOCK), 0, st, in, skey, sidx, tx_head(S), tx_gid(S), n_dev, (const double*)d_cov.p, start_idx, start_cov, (TxGroup*)d_groups.p);
    // per-sample copies: second stable sort by (group, sample)
    hipLaunchKernelGGL(tx_skeys, dim3(grid_for(n_dev)), dim3(TX_BLOCK), 0, st, sidx, tx_gid(S), (const int32_t*)d_graph.p, F.sid_on_device ? (const int32_t*)d_sid.p : (const int32_t*)nullptr, n_dev, (uint64_t*)d_skey.p);
    hipLaunchKernelGGL(tx_iota, dim3(grid_for(n_dev)), dim3(TX_BLOCK), 0, st, (int64_t*)d_pos.p, n_dev);
    { int rc = tx_cub(X.cub_tmp, "sort scratch", [&](void *t, size_t &nb) { return hipcub::DeviceRadixSort::SortPairs(t, nb, (const uint64_t*)d_skey.p, (uint64_t*)d_skey2.p, (const int64_t*)d_pos.p, (int64_t*)d_pos2.p, (int)n_dev, 0, 64, st); }); if(rc != ALD_OK) return rc; }
    hipLaunchKernelGGL(tx_sheads, dim3(grid_for(n_dev)), dim3(TX_BLOCK), 0, st, (const uint64_t*)d_skey2.p, n_dev, (int32_t*)d_head2.p);
    { int rc = tx_cub(X.cub_tmp, "scan scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::InclusiveSum(t, nb, (const int32_t*)d_head2.p, (int32_t*)d_rid.p, (int)n_dev, st); }); if(rc != ALD_OK) return rc; }
    HCHK(hipMemcpyAsync(&F.n_runs, (int32_t*)d_rid.p + (n_dev - 1), 4, hipMemcpyDeviceToHost, st)); tx_count_d2h(S, 4);
    HCHK(hipStreamSynchronize(st));
    if(d_samples.ensure(sizeof(TxSample) * (size_t)F.n_runs)) return ald_set_err(ALD_ERR_NOMEM, "sample records");
    hipLaunchKernelGGL(tx_sfold, dim3(grid_for(n_dev)), dim3(TX_BLOCK), 0, st, in, (const uint64_t*)d_skey2.p, (const int64_t*)d_pos2.p, sidx, (const int32_t*)d_head2.p, (const int32_t*)d_rid.p, n_dev,
                       (const double*)d_cov.p, (TxSample*)d_samples.p);
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a reduction kernel failed to launch");
    return ALD_OK;
}

void tx_host_singles(aletsch::transcript_sink &into, const std::vector<int64_t> &host_paths, const uint32_t *h_pool, const unsigned long long *h_roff,
                     const double *h_cov, const int64_t *h_tid, const int32_t *sid, const int64_t *label, int64_t tid_base, const unsigned long long *h_off)
{
    // one without any exon lands in bucket 0, as get_intron_chain_hashing puts it
    aletsch::sink_transcript x;
    auto rec_at = [&](size_t a) { return h_off ? h_pool + h_off[a] : h_pool + h_roff[(size_t)host_paths[a]]; };
    auto fill = [&](size_t a) {
        const int64_t p = host_paths[a];
        const uint32_t *r = rec_at(a); const int g = (int)r[ALD_REC_GRAPH];
        const double abd = rec_f64(r, ALD_REC_ABD), conf = rec_f64(r, ALD_REC_CONF);
        x.strand = (char)rec_strand(r); x.coverage = h_cov[(size_t)p]; x.top.cov2 = x.coverage; x.top.conf = conf; x.top.abd = abd; x.top.count1 = (int32_t)r[ALD_REC_COUNT]; x.count2 = 1;
        x.tid = h_tid ? h_tid[(size_t)p] : transcript_tid(tid_base, label ? label[g] : (int64_t)g, (int64_t)r[ALD_REC_PATH]);
        const int32_t *ex = rec_exons(r); x.xs.assign(ex, ex + r[ALD_REC_NEXW]);
    };
    for(size_t a = 0; a < host_paths.size(); ) {          // one per-graph set per graph that has any (assembler.cc:1105-1133)
        const int g = (int)rec_at(a)[ALD_REC_GRAPH];
        size_t e = a; while(e < host_paths.size() && (int)rec_at(e)[ALD_REC_GRAPH] == g) e++;
        if(e - a == 1) { fill(a); into.add(x, 1, sid ? sid[g] : -1); }   // merging a one-item set is the same as adding the item (transcript_set.cc:149-175)
        else {
            aletsch::transcript_sink ts(into.single_exon_overlap());
            for(size_t q = a; q < e; q++) { fill(q); ts.add(x, 1, sid ? sid[g] : -1); }
            into.add(ts);
        }
        a = e;
    }
}

// A transcript stream as records of a scratch pool (header + two placeholder vertices + the exon words), groups re-numbered 0 .. G-1 in
// stream order; label[g] = the stream's graph id + graph_offset.  Single-exon transcripts are left out when skip_single_exon.
int tx_stream_records(const uint32_t *words, int64_t n_words, const double *coverage, const int64_t *tid, int32_t skip_single_exon, int64_t graph_offset, StreamRecords &R)
{
    std::vector<uint32_t> &pool = R.pool; std::vector<unsigned long long> &roff = R.roff; std::vector<double> &cov = R.cov; std::vector<int32_t> &sid = R.sid; std::vector<int64_t> &label = R.label, &tids = R.tids;
    int64_t ti = -1;                                       // ti: ordinal of the transcript in the stream (index into `coverage`)
    const int rc = tx_walk_stream(words, n_words, [&](int64_t o, bool first) {
        ti++;
        const uint32_t *w = words + o; const int64_t k = ts_nexw(w);
        if(first) { label.push_back((int64_t)w[ALD_TS_GRAPH] + graph_offset); sid.push_back((int32_t)w[ALD_TS_SID]); }
        if(skip_single_exon && k <= 2) return;
        const size_t at = pool.size(); roff.push_back((unsigned long long)at);
        pool.resize(at + (size_t)rec_words(2, (unsigned)k), 0);
        uint32_t *r = pool.data() + at;
        const int32_t gid1 = (int32_t)label.size();
        for(int l = 0; l < ALD_REC_HDR; l++) r[l] = rec_header_word_of_ts(w, l, &gid1);
        memcpy(r + ALD_REC_HDR + 2, ts_exons(w), 4 * (size_t)k);
        cov.push_back(coverage ? coverage[ti] : log(1.0 + ts_f64(w, ALD_TS_WEIGHT))); if(tid) tids.push_back(tid[ti]);
    });
    if(rc != ALD_OK) return rc;
    R.n_transcripts = ti + 1;
    return ALD_OK;
}

namespace {
// The reduction proper.  d_pool / d_roff: record pool and record offsets in (graph, path) order in HBM; h_pool / h_roff: the same on
// the host (pinned landing areas); h_cov: log(1 + weight) per path (host libm: these values are summed, and the sums are compared bit
// for bit with the host sink); sid: sample of every graph or null; label: graph id that goes into the transcript ids (null: the
// graph index itself); h_tid: explicit transcript id per path (null: tid_base + (label << 20 | path index)).
int reduce_core(RedScratch S, const uint32_t *d_pool, const unsigned long long *d_roff, const uint32_t *h_pool, const unsigned long long *h_roff, const double *h_cov, const int64_t *h_tid,
                int64_t np, int n_graphs, const int32_t *sid, const int64_t *label, int64_t tid_base, int32_t skip_single_exon, double single_exon_overlap, ald_tset_flat **out)
{
    const auto T0 = std::chrono::steady_clock::now();
    std::unique_ptr<ald_tset_flat> Fp(new ald_tset_flat()); ald_tset_flat *F = Fp.get();
    const auto T1 = std::chrono::steady_clock::now();
    // what comes back from the device lands in pinned buffers kept across calls (pageable targets would halve the copy rate, and the
    // device scratch is not reallocated call after call either)
    size_t NGd = 0, NSd = 0; TxFront X;
    const TxGroup *groups = nullptr; const TxSample *samples = nullptr;
    if(np > 0) {
        PinBuf &p_groups = S.x->p_groups, &p_samples = S.x->p_samples;
        hipStream_t st = S.st;
        EventPair ev; HCHK(hipEventCreate(&ev.a)); HCHK(hipEventCreate(&ev.b));
        TxIn in; in.roff = d_roff; in.pool = d_pool; in.np = np;
        X.ev0 = ev.a;
        { int rc = tx_front_groups(S, in, h_cov, n_graphs, sid, X); if(rc != ALD_OK) return rc; }
        if(X.n_dev > 0) {
            { int rc = tx_front_fold(S, in, X, nullptr, nullptr); if(rc != ALD_OK) return rc; }
            if(p_groups.ensure(sizeof(TxGroup) * (size_t)X.n_groups, true) || p_samples.ensure(sizeof(TxSample) * (size_t)X.n_runs, true)) return ald_set_err(ALD_ERR_NOMEM, "pinned reduction buffers");
            NGd = (size_t)X.n_groups; NSd = (size_t)X.n_runs; groups = (const TxGroup*)p_groups.p; samples = (const TxSample*)p_samples.p;
            HCHK(hipMemcpyAsync(p_groups.p, tx_groups(S), sizeof(TxGroup) * NGd, hipMemcpyDeviceToHost, st));
            HCHK(hipMemcpyAsync(p_samples.p, tx_samples(S), sizeof(TxSample) * NSd, hipMemcpyDeviceToHost, st));
        }
        HCHK(hipEventRecord(ev.b, st));
        HCHK(hipStreamSynchronize(st));
        float ms = 0; hipEventElapsedTime(&ms, ev.a, ev.b); F->device_ms = ms;
        if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a reduction kernel failed to launch");
    }
    const auto T2 = std::chrono::steady_clock::now();
    auto graph_label = [&](int g) -> int64_t { return label ? label[g] : (int64_t)g; };
    // ---- host: transcripts with fewer than two exons through the sink (their overlap rule depends on the order of the comparisons)
    aletsch::transcript_sink single(single_exon_overlap);
    if(!skip_single_exon) tx_host_singles(single, X.host_paths, h_pool, h_roff, h_cov, h_tid, sid, label, tid_base);
    const auto T3 = std::chrono::steady_clock::now();
    // ---- host: the flat set.  Device groups arrive in ascending (bucket, key) order, i.e. in the reference's iteration order already;
    // what is left is (i) groups that share a bucket (a 31-bit hash collision): compare1 order among themselves, (ii) the few host
    // items: spliced in by hash, ahead of the device groups of the same bucket (fewer exons sort first, transcript.cc:271)
    const size_t NG = NGd;
    std::vector<int64_t> samp_begin(NG + 1, 0);                    // sample records are sorted by (group, sample id): group k owns [samp_begin[k], samp_begin[k + 1])
    for(size_t q = 0; q < NSd; q++) samp_begin[(size_t)samples[q].gid + 1]++;
    for(size_t k = 0; k < NG; k++) samp_begin[k + 1] += samp_begin[k];
    std::vector<int32_t> order(NG); for(size_t k = 0; k < NG; k++) order[k] = (int32_t)k;
    auto group_exons = [&](const TxGroup &G) { return rec_exons(h_pool + G.first_off); };
    auto group_tx = [&](int k, aletsch::sink_transcript &t) {
        const TxGroup &G = groups[(size_t)k]; const int32_t *x = group_exons(G);
        t.strand = (char)G.strand; t.xs.assign(x, x + G.nw); t.xs.front() = G.lo; t.xs.back() = G.hi;
    };
    for(size_t i = 0; i + 1 < NG; ) {
        size_t j = i + 1; while(j < NG && groups[j].bucket == groups[i].bucket) j++;
        if(j - i > 1) std::stable_sort(order.begin() + (long)i, order.begin() + (long)j, [&](int a, int c) { aletsch::sink_transcript ta, tc; group_tx(a, ta); group_tx(c, tc); return ta.order_against(tc, single_exon_overlap) == +1; });
        i = j;
    }
    const SinkRows hosts = sink_rows(&single, 1);
    const size_t NH = hosts.item.size(), NT = NG + NH;
    // final position of every item: device group at sorted rank q goes behind the host items whose hash does not exceed its bucket (merge_order's rule, over the group records)
    std::vector<int64_t> pos_dev(NG), pos_host(NH);
    { size_t h = 0; for(size_t q = 0; q < NG; q++) { const uint64_t bk = groups[(size_t)order[q]].bucket; while(h < NH && hosts.hash[h] <= bk) { pos_host[h] = (int64_t)(q + h); h++; } pos_dev[q] = (int64_t)(q + h); } while(h < NH) { pos_host[h] = (int64_t)(NG + h); h++; } }
    F->n_device_groups = (int64_t)NG; F->n_host_items = (int64_t)NH;
    flat_resize(*F, (int64_t)NT, 0, 0);
    for(size_t q = 0; q < NG; q++) { const int k = order[q]; F->exon_offset[(size_t)pos_dev[q] + 1] = groups[(size_t)k].nw / 2; F->sample_offset[(size_t)pos_dev[q] + 1] = samp_begin[(size_t)k + 1] - samp_begin[(size_t)k]; }
    for(size_t h = 0; h < NH; h++) { F->exon_offset[(size_t)pos_host[h] + 1] = (int64_t)hosts.item[h]->trst.n_exons(); F->sample_offset[(size_t)pos_host[h] + 1] = (int64_t)hosts.item[h]->samples.size(); }
    for(size_t i = 0; i < NT; i++) { F->exon_offset[i + 1] += F->exon_offset[i]; F->sample_offset[i + 1] += F->sample_offset[i]; }
    flat_resize(*F, (int64_t)NT, F->exon_offset[NT], F->sample_offset[NT]);
    const auto T4 = std::chrono::steady_clock::now();
    unsigned fthr = std::thread::hardware_concurrency(); if(fthr == 0) fthr = 1; if(fthr > 16) fthr = 16; if(NG < 50000) fthr = 1;
    HostBatch::run_threads(fthr, [&](unsigned t) {
        for(size_t q = NG * t / fthr; q < NG * (t + 1) / fthr; q++) {
            const int k = order[q]; const TxGroup &G = groups[(size_t)k]; const size_t i = (size_t)pos_dev[q];
            F->hash[i] = G.bucket; F->count[i] = G.count; F->strand[i] = (char)G.strand; F->coverage[i] = G.coverage; F->cov2[i] = G.cov2; F->conf[i] = G.conf; F->abd[i] = G.abd; F->count1[i] = G.count1;
            F->tid[i] = h_tid ? h_tid[(size_t)G.first] : transcript_tid(tid_base, graph_label(G.graph), (int64_t)G.path);
            int32_t *e = &F->exon_lr[2 * (size_t)F->exon_offset[i]];
            memcpy(e, group_exons(G), 4 * (size_t)G.nw); e[0] = G.lo; e[G.nw - 1] = G.hi;
            size_t so = (size_t)F->sample_offset[i]; int c2 = 0;
            for(int64_t sx = samp_begin[(size_t)k]; sx < samp_begin[(size_t)k + 1]; sx++, so++, c2++) {
                const TxSample &Sm = samples[(size_t)sx];
                F->sample_sid[so] = Sm.sid; F->sample_cov2[so] = Sm.cov2; F->sample_conf[so] = Sm.conf; F->sample_abd[so] = Sm.abd; F->sample_count1[so] = Sm.count1;
            }
            F->count2[i] = c2;
        }
    });
    { const FlatMut V = flat_mut(*F); for(size_t h = 0; h < NH; h++) flat_put_item(V, pos_host[h], hosts.hash[h], *hosts.item[h]); }
    F->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    if(getenv("ALD_SINK_PROF")) { auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) { return std::chrono::duration<double, std::milli>(c - a).count(); };
        fprintf(stderr, "[reduce] setup %.1f ms, device section %.1f ms (events %.1f), single-exon host %.1f ms, order + offsets %.1f ms, fill %.1f ms\n", ms(T0, T1), ms(T1, T2), F->device_ms, ms(T2, T3), ms(T3, T4), ms(T4, std::chrono::steady_clock::now())); }
    *out = Fp.release();
    return ALD_OK;
}
} // namespace

extern "C" {

int ald_batch_reduce_transcripts(const ald_batch *cb, const int32_t *sid, int64_t tid_base, int32_t skip_single_exon, double single_exon_overlap, ald_tset_flat **out)
{
    if(!cb || !out) return ALD_ERR_INVALID;
    if(!cb->downloaded) return ald_set_err(ALD_ERR_STATE, "ald_batch_reduce_transcripts before ald_batch_download");
    ald_batch *b = const_cast<ald_batch*>(cb);
    HCHK(hipSetDevice(b->device));
    { int rc = device_path_table(b); if(rc != ALD_OK) return rc; }
    const int64_t np = b->total_paths;
    // the host's side: the record pool is in the batch's pinned landing area, the offsets in (graph, path) order and the coverages
    // (log(1 + weight), host libm) are the path table ald_batch_download built from the kernel's index
    const unsigned long long *h_roff = (const unsigned long long*)b->res.rec_off.data(); const double *h_cov = b->res.coverage.data();
    RedScratch S; S.x = &b->tx; S.st = b->stream;
    return reduce_core(S, (const uint32_t*)b->d_pool.p, (const unsigned long long*)b->d_ordoff.p, b->res.pool_data(), h_roff, h_cov, nullptr, np, b->hb.n(), sid, nullptr, tid_base, skip_single_exon, single_exon_overlap, out);
}

// The same reduction fed with a TRANSCRIPT STREAM (the format of ald_batch_transcript_stream; groups = runs of equal graph id, in
// ascending order) instead of a decomposed batch: the transcripts become records of a scratch pool, go to the device and through
// the very kernels a batch's records go through.  This is how transcripts that did not come out of the decomposition kernel -- the
// reference-generated cases of tests/golden/ref_tset.json, a stream received from another rank -- reach the device stage.
int ald_tset_reduce_stream(int32_t device, const uint32_t *words, int64_t n_words, const double *coverage, const int64_t *tid, int64_t tid_base, int32_t skip_single_exon, double single_exon_overlap, ald_tset_flat **out)
{
    if(!out || n_words < 0 || (n_words > 0 && !words)) return ALD_ERR_INVALID;
    { int rc = tx_need_device(device, "the reduction"); if(rc != ALD_OK) return rc; }
    HCHK(hipSetDevice(device));
    StreamRecords R;
    { int rc = tx_stream_records(words, n_words, coverage, tid, skip_single_exon, 0, R); if(rc != ALD_OK) return rc; }
    std::vector<uint32_t> &pool = R.pool; std::vector<unsigned long long> &roff = R.roff; std::vector<double> &cov = R.cov; std::vector<int32_t> &sid = R.sid; std::vector<int64_t> &label = R.label, &tids = R.tids;
    const int64_t np = (int64_t)roff.size();
    Scoped<TxScratch> tx; Scoped<DevBuf> d_pool, d_roff;
    ScopedStream stream; HCHK(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    hipStream_t st = stream.s;
    if(np > 0) {
        if(d_pool.ensure(4 * pool.size() + 64) || d_roff.ensure(8 * (size_t)np + 8)) return ald_set_err(ALD_ERR_NOMEM, "stream reduction buffers");
        HCHK(hipMemcpyAsync(d_pool.p, pool.data(), 4 * pool.size(), hipMemcpyHostToDevice, st));
        HCHK(hipMemcpyAsync(d_roff.p, roff.data(), 8 * (size_t)np, hipMemcpyHostToDevice, st));
        HCHK(hipStreamSynchronize(st));
    }
    RedScratch S; S.x = &tx; S.st = st;
    return reduce_core(S, (const uint32_t*)d_pool.p, (const unsigned long long*)d_roff.p, pool.data(), roff.data(), cov.data(), tid ? tids.data() : nullptr, np, (int)label.size(), sid.empty() ? nullptr : sid.data(), label.data(), tid_base, 0 /* filtered above */, single_exon_overlap, out);
}

// The stream of ald_batch_transcript_stream, word for word, built on the device and left there: a rank hands it to RCCL without the
// 200 MB making a round trip through host memory.  Nothing comes from the host: the record offsets in (graph, path) order are
// derived on the device from the index the decomposition kernel wrote (device_path_table), the exons are in the records; one
// number comes back, the length.
int ald_batch_device_transcript_stream(const ald_batch *cb, const int32_t *sid, int32_t skip_single_exon, void **dev_words, int64_t *n_words)
{
    if(!cb || !dev_words || !n_words) return ALD_ERR_INVALID;
    if(!cb->downloaded && !cb->finished) return ald_set_err(ALD_ERR_STATE, "ald_batch_device_transcript_stream before ald_batch_download / ald_batch_finish");
    ald_batch *b = const_cast<ald_batch*>(cb);
    HCHK(hipSetDevice(b->device));
    const int n = b->hb.n(); const int64_t np = b->total_paths;
    *dev_words = nullptr; *n_words = 0;
    if(np == 0) return ALD_OK;
    { int rc = device_path_table(b); if(rc != ALD_OK) return rc; }
    PinBuf &p_tot = b->tx.p_count;
    DevBuf &d_sid = b->tx.sid;
    DevBuf &d_len = b->d_ts_len, &d_at = b->d_ts_at, &d_out = b->d_ts_out;
    if(p_tot.ensure(64)) return ald_set_err(ALD_ERR_NOMEM, "pinned counter");
    if(d_len.ensure(8 * (size_t)std::max<int64_t>(np, n) + 8) || d_at.ensure(8 * (size_t)np + 8) || (sid && d_sid.ensure(4 * (size_t)n + 4))) return ald_set_err(ALD_ERR_NOMEM, "transcript stream buffers");
    hipStream_t st = b->stream;
    if(sid) HCHK(hipMemcpyAsync(d_sid.p, sid, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    TxIn in; in.roff = (const unsigned long long*)b->d_ordoff.p; in.pool = (const uint32_t*)b->d_pool.p; in.np = np;
    hipLaunchKernelGGL(ts_len, dim3(grid_for(np + 1)), dim3(TX_BLOCK), 0, st, in, (int)(skip_single_exon != 0), (int64_t*)d_len.p);
    { int rc = tx_cub(b->tx.cub_tmp, "scan scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int64_t*)d_len.p, (int64_t*)d_at.p, (int)(np + 1), st); }); if(rc != ALD_OK) return rc; }
    HCHK(hipMemcpyAsync(p_tot.p, (const int64_t*)d_at.p + np, 8, hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    const int64_t total = *(const int64_t*)p_tot.p;
    if(d_out.ensure(4 * (size_t)total + 64)) return ald_set_err(ALD_ERR_NOMEM, "transcript stream");
    hipLaunchKernelGGL(ts_emit, dim3(grid_for(16 * np)), dim3(TX_BLOCK), 0, st, in, (const int64_t*)d_at.p, sid ? (const int32_t*)d_sid.p : (const int32_t*)nullptr, (uint32_t*)d_out.p);
    HCHK(hipStreamSynchronize(st));
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a transcript-stream kernel failed to launch");
    *dev_words = d_out.p; *n_words = total;
    return ALD_OK;
}

int ald_tset_flat_size(const ald_tset_flat *f, int64_t *n_items, int64_t *n_exons, int64_t *n_samples)
{
    if(!f) return ALD_ERR_INVALID;
    if(n_items) *n_items = (int64_t)f->hash.size(); if(n_exons) *n_exons = (int64_t)f->exon_lr.size() / 2; if(n_samples) *n_samples = (int64_t)f->sample_sid.size();
    return ALD_OK;
}
int ald_tset_flat_stats(const ald_tset_flat *f, double *device_ms, double *total_ms, int64_t *device_groups, int64_t *host_items)
{
    if(!f) return ALD_ERR_INVALID;
    if(device_ms) *device_ms = f->device_ms; if(total_ms) *total_ms = f->host_ms; if(device_groups) *device_groups = f->n_device_groups; if(host_items) *host_items = f->n_host_items;
    return ALD_OK;
}
int ald_tset_flat_export(const ald_tset_flat *f, uint64_t *hash, int32_t *count, char *strand, double *coverage, double *cov2, double *conf, double *abd,
                         int32_t *count1, int32_t *count2, int64_t *tid, int64_t *exon_offset, int32_t *exon_lr,
                         int64_t *sample_offset, int32_t *sample_sid, double *sample_cov2, double *sample_conf, double *sample_abd, int32_t *sample_count1)
{
    if(!f) return ALD_ERR_INVALID;
    const FlatView src = flat_view(*f);
    const FlatMut dst{hash, count, strand, coverage, cov2, conf, abd, count1, count2, tid, exon_offset, exon_lr, sample_offset, sample_sid, sample_cov2, sample_conf, sample_abd, sample_count1, src.n, src.ne, src.ns};
    if(flat_has_null(dst)) return ALD_ERR_INVALID;
    flat_copy(dst, src);
    return ALD_OK;
}
int ald_tset_flat_free(ald_tset_flat *f) { delete f; return ALD_OK; }

// transcript_set::add(transcript_set &) (transcript_set.cc:156-175): the reduced set of a batch merged into a persistent one, bucket by bucket
int ald_tset_add_flat(ald_tset *t, const ald_tset_flat *f)
{
    if(!t || !f) return ALD_ERR_INVALID;
    const FlatView v = flat_view(*f); const size_t n = (size_t)v.n;
    // buckets never interact and bucket h lives in table h % ALD_TSET_SHARDS: thread th zips the buckets of ITS tables (every thread
    // scans the hashes, which are ascending; building the items is the work)
    const unsigned nthr = ald_sink_threads((int64_t)n);
    HostBatch::run_threads(nthr, [&](unsigned th) {
        for(size_t i = 0; i < n; ) {
            size_t j = i + 1; while(j < n && f->hash[j] == f->hash[i]) j++;
            if((f->hash[i] % ALD_TSET_SHARDS) % nthr != th) { i = j; continue; }
            aletsch::transcript_sink::bucket vec;
            for(size_t k = i; k < j; k++) vec.push_back(flat_get_item(v, (int64_t)k));
            t->shard[f->hash[i] % ALD_TSET_SHARDS].add_bucket((size_t)f->hash[i], vec);
            i = j;
        }
    });
    return ALD_OK;
}

} // extern "C"
