// tset_resident.hip -- a transcript set that lives in HBM: batches (or transcript streams) fold into it on the device, call after call,
// and it leaves the device only when the caller asks (ald_tset_dev_*).
//
// What it replaces: the region's `tm` of meta/assembler.cc:1105-1133 -- per graph ts.add(t, 1, sid), then tm.add(ts) into a set that is
// NOT empty (rnacore/transcript_set.cc:149-175) -- and transcript_set::add(transcript_set&) between two such sets.  tset_reduce.hip
// folds a batch into an EMPTY set; here the batch's groups meet the resident items, which changes exactly one thing: a group that lands
// on a resident item of coverage c sums ((c + s1) + s2) + ..., not c + (s1 + s2 + ...), so the fold starts from the resident value.
// Everything else a merge computes (counts, maxima, bounds, the union of the per-sample maps) does not depend on the order.
//
// Layout: structure of arrays sorted by (bucket hash, compare1), exons and samples as CSR (samples sorted by sid; count2 and the
// per-sample coverage are derived: #samples and the item's coverage, transcript_set.cc:70-74).  Two buffer sets: every add writes the
// other one and swaps, so a failed allocation leaves the set as it was.  Transcripts with fewer than two exons merge by an overlap test
// that is not transitive; they stay in a host transcript_sink inside the set, fed graph by graph, and are spliced in by hash on export.
//
// One add (HBM-bound streaming passes; one lane per item):
//   front end (tset_reduce.hip: tx_build, radix sort, tx_heads)   the batch's multi-exon groups
//   rs_ghead / rs_order    groups in (bucket, compare1) order: the sort key orders by bucket; a lane per equal-bucket run sorts it
//   rs_match               binary search on the resident hashes, then a compare1 walk inside the bucket: match or insertion point
//   tx_fold (with start)   coverage from the matched item's value in (graph, path) order; tx_sfold: per-sample maxima
//   rs_mark / scans / rs_slots   merge path: resident i -> i + #new before it, new j -> insertion point + #new before j
//   rs_sizes / scans / rs_write  exon and sample counts per output item, prefix sums, then one gather pass into the other buffer set
// ald_tset_dev_merge runs the same merge path with a second resident set as the incoming side (coverage c_dst + c_src).
// A batch that ald_batch_finish ended has no host copy of its records: the front end then runs in its halves (tset_front.h: tx_front_sort /
// _coverage / _heads) -- the key pass also writes the weights, the host takes log(1 + w) under the sort -- and the single-exon records
// the host part merges are compacted on the device (tx_compact_singles).
// A stream in DEVICE memory (a segment the owner exchange left there) takes the same form: its transcript boundaries come from the stream
// index (tset_index.hip), then
//   sr_len / scans         which transcripts stay (skip_single_exon), where their scratch records begin, their ordinal among the kept
//   sr_emit                16 lanes / transcript: the scratch record tx_stream_records would build, word for word, straight into d_pool;
//                          the caller's coverage / tid (uploaded, indexed by stream ordinal) gathered to the kept ordinal
// so no word of the stream reaches host memory: per call the counts, label / sid per group, and what a finished batch brings.
#include "tset_front.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <chrono>
#include <memory>

namespace {

struct SetView {                     // one buffer set as the kernels see it (n items)
    uint64_t *hash; int32_t *count; int8_t *strand; double *cov, *cov2, *conf, *abd; int32_t *count1; int64_t *tid;
    int64_t *eoff; int32_t *lr;      // exons of item i: lr[2 * eoff[i] .. 2 * eoff[i + 1]) (l, r pairs)
    int64_t *soff; int32_t *ssid, *sc1; double *scov2, *sconf, *sabd;      // samples of item i: [soff[i], soff[i + 1]), ascending sid
    int64_t n;
};

struct SetBufs {
    DevBuf hash, count, strand, cov, cov2, conf, abd, count1, tid, eoff, lr, soff, ssid, sc1, scov2, sconf, sabd;
    int64_t n = 0, ne = 0, ns = 0;   // items, exons, samples
    SetView view() {
        SetView v; v.hash = (uint64_t*)hash.p; v.count = (int32_t*)count.p; v.strand = (int8_t*)strand.p; v.cov = (double*)cov.p; v.cov2 = (double*)cov2.p; v.conf = (double*)conf.p;
        v.abd = (double*)abd.p; v.count1 = (int32_t*)count1.p; v.tid = (int64_t*)tid.p; v.eoff = (int64_t*)eoff.p; v.lr = (int32_t*)lr.p; v.soff = (int64_t*)soff.p;
        v.ssid = (int32_t*)ssid.p; v.sc1 = (int32_t*)sc1.p; v.scov2 = (double*)scov2.p; v.sconf = (double*)sconf.p; v.sabd = (double*)sabd.p; v.n = n; return v;
    }
    // the same buffers under the names of the flat set's columns (tset_flat.h; DEVICE pointers).  count2 is not stored: #samples
    FlatView flat() const { return FlatView{(const uint64_t*)hash.p, (const int32_t*)count.p, (const char*)strand.p, (const double*)cov.p, (const double*)cov2.p, (const double*)conf.p, (const double*)abd.p, (const int32_t*)count1.p, nullptr,
                        (const int64_t*)tid.p, (const int64_t*)eoff.p, (const int32_t*)lr.p, (const int64_t*)soff.p, (const int32_t*)ssid.p, (const double*)scov2.p, (const double*)sconf.p, (const double*)sabd.p, (const int32_t*)sc1.p, n, ne, ns}; }
    int ensure_items(int64_t k) {    // k items (+1 offset entry)
        const size_t m = (size_t)k + 1;
        return hash.ensure(8 * m) || count.ensure(4 * m) || strand.ensure(m) || cov.ensure(8 * m) || cov2.ensure(8 * m) || conf.ensure(8 * m) || abd.ensure(8 * m)
               || count1.ensure(4 * m) || tid.ensure(8 * m) || eoff.ensure(8 * m) || soff.ensure(8 * m);
    }
    int ensure_tail(int64_t n_exons, int64_t n_samples) {
        const size_t e = (size_t)n_exons + 1, s = (size_t)n_samples + 1;
        return lr.ensure(8 * e) || ssid.ensure(4 * s) || sc1.ensure(4 * s) || scov2.ensure(8 * s) || sconf.ensure(8 * s) || sabd.ensure(8 * s);
    }
    void release() { DevBuf *all[] = {&hash, &count, &strand, &cov, &cov2, &conf, &abd, &count1, &tid, &eoff, &lr, &soff, &ssid, &sc1, &scov2, &sconf, &sabd}; for(DevBuf *d : all) d->release(); n = ne = ns = 0; }
};

// transcript::compare1 for two chains of >= 2 exons (transcript.cc:269-300): +1 when a sorts first, -1 when b does, 0 equal.  The
// words looked at: 1, 2 .. nw-5, nw-2 (intron_chain_compare stops one exon early and never sees the outer bounds, transcript.cc:218-238)
__device__ inline int cmp1(int na, int sa, const int32_t *xa, int nb, int sb, const int32_t *xb)
{
    if(na != nb) return na < nb ? 1 : -1;
    if(sa != sb) return sa < sb ? 1 : -1;
    if(xa[1] != xb[1]) return xa[1] < xb[1] ? 1 : -1;
    for(int k = 2; k + 5 <= na; k++) if(xa[k] != xb[k]) return xa[k] < xb[k] ? 1 : -1;
    if(xa[na - 2] != xb[na - 2]) return xa[na - 2] < xb[na - 2] ? 1 : -1;
    return 0;
}
__device__ inline int rec_strand_char(const uint32_t *r) { return (int)(int8_t)rec_strand(r); }      // the reference's `char` strand

// The incoming side of a merge, two kinds with one interface.  j: position in (hash, compare1) order.
struct InBatch {                     // a batch's groups: before the fold only hash / nw / strand / x are valid (they come from the records)
    TxIn in; const int64_t *sidx; const int32_t *ghead; const uint64_t *skey; const int32_t *perm;
    const TxGroup *grp; const TxSample *smp; const int64_t *sbeg;
    int64_t tid_base; const int64_t *label, *ptid; int64_t n;
    __device__ const uint32_t *rec(int64_t j) const { return in.pool + in.roff[sidx[ghead[perm[j]]]]; }
    __device__ uint64_t hash(int64_t j) const { return skey[ghead[perm[j]]] >> 32; }
    __device__ int nw(int64_t j) const { return (int)rec(j)[ALD_REC_NEXW]; }
    __device__ int strand(int64_t j) const { return rec_strand_char(rec(j)); }
    __device__ const int32_t *x(int64_t j) const { return rec_exons(rec(j)); }
    __device__ int32_t lo(int64_t j) const { return grp[perm[j]].lo; }
    __device__ int32_t hi(int64_t j) const { return grp[perm[j]].hi; }
    __device__ int32_t count(int64_t j) const { return grp[perm[j]].count; }
    __device__ double cov(int64_t j) const { return grp[perm[j]].coverage; }
    __device__ double matched_cov(int64_t j, double) const { return grp[perm[j]].coverage; }     // the fold started from the resident value
    __device__ double cov2(int64_t j) const { return grp[perm[j]].cov2; }
    __device__ double conf(int64_t j) const { return grp[perm[j]].conf; }
    __device__ double abd(int64_t j) const { return grp[perm[j]].abd; }
    __device__ int32_t count1(int64_t j) const { return grp[perm[j]].count1; }
    __device__ int64_t tid(int64_t j) const { const TxGroup &G = grp[perm[j]]; return ptid ? ptid[G.first] : transcript_tid(tid_base, label ? label[G.graph] : (int64_t)G.graph, (int64_t)G.path); }
    __device__ int64_t sb(int64_t j) const { return sbeg[perm[j]]; }
    __device__ int64_t se(int64_t j) const { return sbeg[perm[j] + 1]; }
    __device__ void sample(int64_t s, int32_t &sid, double &c2, double &cf, double &ab, int32_t &c1) const { const TxSample &S = smp[s]; sid = S.sid; c2 = S.cov2; cf = S.conf; ab = S.abd; c1 = S.count1; }
};
struct InSet {                       // a second resident set (ald_tset_dev_merge)
    SetView v; int64_t n;
    __device__ uint64_t hash(int64_t j) const { return v.hash[j]; }
    __device__ int nw(int64_t j) const { return (int)(2 * (v.eoff[j + 1] - v.eoff[j])); }
    __device__ int strand(int64_t j) const { return (int)v.strand[j]; }
    __device__ const int32_t *x(int64_t j) const { return v.lr + 2 * v.eoff[j]; }
    __device__ int32_t lo(int64_t j) const { return x(j)[0]; }
    __device__ int32_t hi(int64_t j) const { return x(j)[nw(j) - 1]; }
    __device__ int32_t count(int64_t j) const { return v.count[j]; }
    __device__ double cov(int64_t j) const { return v.cov[j]; }
    __device__ double matched_cov(int64_t j, double c) const { return c + v.cov[j]; }          // trans_item::merge of two finished items
    __device__ double cov2(int64_t j) const { return v.cov2[j]; }
    __device__ double conf(int64_t j) const { return v.conf[j]; }
    __device__ double abd(int64_t j) const { return v.abd[j]; }
    __device__ int32_t count1(int64_t j) const { return v.count1[j]; }
    __device__ int64_t tid(int64_t j) const { return v.tid[j]; }
    __device__ int64_t sb(int64_t j) const { return v.soff[j]; }
    __device__ int64_t se(int64_t j) const { return v.soff[j + 1]; }
    __device__ void sample(int64_t s, int32_t &sid, double &c2, double &cf, double &ab, int32_t &c1) const { sid = v.ssid[s]; c2 = v.scov2[s]; cf = v.sconf[s]; ab = v.sabd[s]; c1 = v.sc1[s]; }
};

__device__ inline int64_t lane_id() { return (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x; }

// ---- a device stream as scratch records (tx_stream_records on the device).  keep[i]: transcript i stays; len[i]: words of its record
__global__ void sr_len(const uint32_t *words, const unsigned long long *toff, int64_t nt, int skip_single, int64_t *len, int32_t *keep)
{
    const int64_t i = lane_id();
    if(i > nt) return;
    if(i == nt) { len[i] = 0; keep[i] = 0; return; }        // (the exclusive scans over nt + 1 entries leave the totals in the last one)
    const int64_t k = 2 * (int64_t)words[toff[i] + ALD_TS_NEXONS];
    const bool kp = !(skip_single && k <= 2);
    len[i] = kp ? (int64_t)rec_words(2, (unsigned)k) : 0; keep[i] = kp ? 1 : 0;
}
// header + two placeholder vertices + the exon words (18 + k words: even, so no padding word), consecutive lanes on consecutive words
__global__ void sr_emit(const uint32_t *words, const unsigned long long *toff, const int32_t *gid, const int64_t *at, const int32_t *kord, int64_t nt,
                        const double *cov_in, const int64_t *tid_in, uint32_t *pool, unsigned long long *roff, double *cov, int64_t *tid)
{
    const int64_t i = lane_id() / 16; const int l = (int)(threadIdx.x & 15);
    if(i >= nt) return;
    const int64_t o = at[i];
    if(at[i + 1] == o) return;
    const uint32_t *w = words + toff[i]; uint32_t *r = pool + o;
    const int k = 2 * (int)w[ALD_TS_NEXONS];
    r[l] = rec_header_word_of_ts(w, l, gid + i);
    if(l < 2) r[ALD_REC_HDR + l] = 0;
    for(int q = l; q < k; q += 16) r[ALD_REC_HDR + 2 + q] = w[ALD_TS_HDR + q];
    if(l == 0) { const int32_t p = kord[i]; roff[p] = (unsigned long long)o; if(cov_in) cov[p] = cov_in[i]; if(tid_in) tid[p] = tid_in[i]; }
}

// head position (in the sorted member order) of every group
__global__ void rs_ghead(const int32_t *head, const int32_t *gid, int64_t n_dev, int32_t *ghead)
{
    const int64_t i = lane_id();
    if(i < n_dev && head[i]) ghead[gid[i] - 1] = (int32_t)i;
}
// groups come out of the front end ordered by (bucket, 32-bit group hash); compare1 order inside a bucket: the first lane of every
// equal-bucket run sorts the run (nearly always of length 1) by insertion
__global__ void rs_order(TxIn in, const int64_t *sidx, const int32_t *ghead, const uint64_t *skey, int64_t n_groups, int32_t *perm)
{
    const int64_t k = lane_id();
    if(k >= n_groups) return;
    const uint64_t bk = skey[ghead[k]] >> 32;
    if(k > 0 && (skey[ghead[k - 1]] >> 32) == bk) return;
    int64_t e = k + 1; while(e < n_groups && (skey[ghead[e]] >> 32) == bk) e++;
    for(int64_t q = k; q < e; q++) perm[q] = (int32_t)q;
    for(int64_t q = k + 1; q < e; q++) {
        const int32_t v = perm[q]; const uint32_t *rv = in.pool + in.roff[sidx[ghead[v]]];
        int64_t p = q;
        while(p > k) {
            const uint32_t *ru = in.pool + in.roff[sidx[ghead[perm[p - 1]]]];
            if(cmp1((int)rv[ALD_REC_NEXW], rec_strand_char(rv), rec_exons(rv), (int)ru[ALD_REC_NEXW], rec_strand_char(ru), rec_exons(ru)) != 1) break;
            perm[p] = perm[p - 1]; p--;
        }
        perm[p] = v;
    }
}
// match or insertion point of incoming item j in the resident set A; unm[j] = 1 for an item A does not have (unm[n] = 0 for the scan)
template<class In> __global__ void rs_match(SetView A, In B, int64_t *match, int64_t *ins, int32_t *unm)
{
    const int64_t j = lane_id();
    if(j > B.n) return;
    if(j == B.n) { unm[j] = 0; return; }
    const uint64_t h = B.hash(j);
    int64_t lo = 0, hi = A.n;
    while(lo < hi) { const int64_t m = (lo + hi) >> 1; if(A.hash[m] < h) lo = m + 1; else hi = m; }
    const int nb = B.nw(j), sb = B.strand(j); const int32_t *xb = B.x(j);
    int64_t p = lo; int c = 1;
    while(p < A.n && A.hash[p] == h && (c = cmp1((int)(2 * (A.eoff[p + 1] - A.eoff[p])), (int)A.strand[p], A.lr + 2 * A.eoff[p], nb, sb, xb)) == 1) p++;
    const bool hit = p < A.n && A.hash[p] == h && c == 0;
    match[j] = hit ? p : -1; ins[j] = p; unm[j] = hit ? 0 : 1;
}
__global__ void rs_start(const int32_t *perm, const int64_t *match, int64_t n, int64_t *start_idx)
{
    const int64_t j = lane_id();
    if(j < n) start_idx[perm[j]] = match[j];
}
// resident item -> the incoming item that lands on it; per resident position the number of new items placed in front of it
__global__ void rs_mark(const int64_t *match, const int64_t *ins, int64_t n, int64_t *rmatch, int32_t *cnt)
{
    const int64_t j = lane_id();
    if(j >= n) return;
    if(match[j] >= 0) rmatch[match[j]] = j; else atomicAdd(&cnt[ins[j]], 1);
}
// output slot of every item: slot[o] = i (resident) or -(j + 1) (new); shift: inclusive scan of cnt, ub: exclusive scan of unm
__global__ void rs_slots(int64_t nA, int64_t nB, const int32_t *shift, const int64_t *match, const int64_t *ins, const int32_t *ub, int64_t *slot)
{
    const int64_t t = lane_id();
    if(t < nA) slot[t + shift[t]] = t;
    else if(t < nA + nB) { const int64_t j = t - nA; if(match[j] < 0) slot[ins[j] + ub[j]] = -(j + 1); }
}
// the union of two ascending sid lists; emit(sid, from_a, ia, from_b, ib) once per distinct sid
template<class In, class F> __device__ inline void sample_union(const SetView &A, int64_t i, const In &B, int64_t j, F emit)
{
    int64_t a = A.soff[i], ae = A.soff[i + 1], b = B.sb(j), be = B.se(j);
    int32_t bs = 0, c1; double c2, cf, ab;
    if(b < be) B.sample(b, bs, c2, cf, ab, c1);
    while(a < ae || b < be) {
        if(b >= be || (a < ae && A.ssid[a] < bs)) { emit(true, a, false, b); a++; }
        else if(a >= ae || bs < A.ssid[a]) { emit(false, a, true, b); b++; if(b < be) B.sample(b, bs, c2, cf, ab, c1); }
        else { emit(true, a, true, b); a++; b++; if(b < be) B.sample(b, bs, c2, cf, ab, c1); }
    }
}
template<class In> __global__ void rs_sizes(SetView A, In B, const int64_t *slot, const int64_t *rmatch, int64_t N, int64_t *ecnt, int64_t *scnt)
{
    const int64_t o = lane_id();
    if(o > N) return;
    if(o == N) { ecnt[o] = 0; scnt[o] = 0; return; }
    const int64_t s = slot[o];
    if(s >= 0) {
        const int64_t j = rmatch[s];
        ecnt[o] = A.eoff[s + 1] - A.eoff[s];
        if(j < 0) scnt[o] = A.soff[s + 1] - A.soff[s];
        else { int64_t k = 0; sample_union(A, s, B, j, [&](bool, int64_t, bool, int64_t) { k++; }); scnt[o] = k; }
    } else {
        const int64_t j = -s - 1;
        ecnt[o] = B.nw(j) / 2; scnt[o] = B.se(j) - B.sb(j);
    }
}
// the gather: every output item from its resident item (+ the incoming item that lands on it) or from a new incoming item.  Maxima are
// raised resident-first, as trans_item::merge raises the item that was there (transcript_set.cc:47-50, 63-66)
template<class In> __global__ void rs_write(SetView A, In B, const int64_t *slot, const int64_t *rmatch, int64_t N, SetView O)
{
    const int64_t o = lane_id();
    if(o >= N) return;
    const int64_t s = slot[o];
    int32_t *ox = O.lr + 2 * O.eoff[o]; int64_t so = O.soff[o];
    if(s >= 0) {
        const int64_t j = rmatch[s];
        const int nw = (int)(2 * (A.eoff[s + 1] - A.eoff[s])); const int32_t *ax = A.lr + 2 * A.eoff[s];
        for(int q = 0; q < nw; q++) ox[q] = ax[q];
        O.hash[o] = A.hash[s]; O.strand[o] = A.strand[s]; O.tid[o] = A.tid[s];
        int32_t cnt = A.count[s], c1 = A.count1[s]; double cov = A.cov[s], c2 = A.cov2[s], cf = A.conf[s], ab = A.abd[s];
        if(j < 0) {
            for(int64_t q = A.soff[s]; q < A.soff[s + 1]; q++, so++) { O.ssid[so] = A.ssid[q]; O.scov2[so] = A.scov2[q]; O.sconf[so] = A.sconf[q]; O.sabd[so] = A.sabd[q]; O.sc1[so] = A.sc1[q]; }
        } else {
            cnt += B.count(j); cov = B.matched_cov(j, cov);
            if(c2 < B.cov2(j)) c2 = B.cov2(j); if(cf < B.conf(j)) cf = B.conf(j); if(ab < B.abd(j)) ab = B.abd(j); if(c1 < B.count1(j)) c1 = B.count1(j);
            if(B.lo(j) < ox[0]) ox[0] = B.lo(j); if(B.hi(j) > ox[nw - 1]) ox[nw - 1] = B.hi(j);
            sample_union(A, s, B, j, [&](bool ina, int64_t a, bool inb, int64_t b) {
                int32_t sid, k1; double k2, kf, kb;
                if(ina) { sid = A.ssid[a]; k2 = A.scov2[a]; kf = A.sconf[a]; kb = A.sabd[a]; k1 = A.sc1[a]; }
                if(inb) {
                    int32_t bs, b1; double b2, bf, bb; B.sample(b, bs, b2, bf, bb, b1);
                    if(!ina) { sid = bs; k2 = b2; kf = bf; kb = bb; k1 = b1; }
                    else { if(k2 < b2) k2 = b2; if(kf < bf) kf = bf; if(kb < bb) kb = bb; if(k1 < b1) k1 = b1; }
                }
                O.ssid[so] = sid; O.scov2[so] = k2; O.sconf[so] = kf; O.sabd[so] = kb; O.sc1[so] = k1; so++;
            });
        }
        O.count[o] = cnt; O.cov[o] = cov; O.cov2[o] = c2; O.conf[o] = cf; O.abd[o] = ab; O.count1[o] = c1;
    } else {
        const int64_t j = -s - 1;
        const int nw = B.nw(j); const int32_t *bx = B.x(j);
        for(int q = 0; q < nw; q++) ox[q] = bx[q];
        ox[0] = B.lo(j); ox[nw - 1] = B.hi(j);
        O.hash[o] = B.hash(j); O.strand[o] = (int8_t)B.strand(j); O.tid[o] = B.tid(j);
        O.count[o] = B.count(j); O.cov[o] = B.cov(j); O.cov2[o] = B.cov2(j); O.conf[o] = B.conf(j); O.abd[o] = B.abd(j); O.count1[o] = B.count1(j);
        for(int64_t q = B.sb(j); q < B.se(j); q++, so++) {
            int32_t sid, k1; double k2, kf, kb; B.sample(q, sid, k2, kf, kb, k1);
            O.ssid[so] = sid; O.scov2[so] = k2; O.sconf[so] = kf; O.sabd[so] = kb; O.sc1[so] = k1;
        }
    }
}
// first sample run of every group (runs are sorted by group): sbeg[k] = lower bound of k in the runs' group ids
__global__ void rs_sbeg(const TxSample *smp, int64_t n_runs, int64_t n_groups, int64_t *sbeg)
{
    const int64_t k = lane_id();
    if(k > n_groups) return;
    int64_t lo = 0, hi = n_runs;
    while(lo < hi) { const int64_t m = (lo + hi) >> 1; if(smp[m].gid < k) lo = m + 1; else hi = m; }
    sbeg[k] = lo;
}

} // namespace

struct ald_tset_dev {
    int device = 0; hipStream_t st = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_w = nullptr;                              // behind the D2H of a finished batch's weights (tx_front_sort)
    SetBufs buf[2]; int cur = 0;
    aletsch::transcript_sink single;                        // transcripts with fewer than two exons, in call order
    TxScratch tx; DevBuf d_pool, d_roff, d_label, d_tid;    // front end scratch (the set's own, never a batch's)
    MergeScratch mg;                                        // merge-path scratch
    StreamIndexScratch ix; StreamRecScratch sr;             // a device stream: the stream index, the record build (sr_len / sr_emit)
    hipEvent_t ev_i0 = nullptr, ev_i1 = nullptr;            // around the index kernels
    double last_device_ms = 0, last_call_ms = 0;
    // of the last ald_tset_dev_add_stream (ald_tset_dev_stream_stats)
    int64_t st_transcripts = 0, st_groups = 0, st_words_to_host = 0, bytes_to_host = 0; double st_index_ms = 0;
    explicit ald_tset_dev(double ov) : single(ov) {}
    SetBufs &res() { return buf[cur]; }
    const SetBufs &res() const { return buf[cur]; }
    ~ald_tset_dev() {
        for(auto &b : buf) b.release();
        tx.release(); mg.release(); ix.release(); sr.release();
        if(ev_i0) hipEventDestroy(ev_i0); if(ev_i1) hipEventDestroy(ev_i1);
        d_pool.release(); d_roff.release(); d_label.release(); d_tid.release();
        if(ev0) hipEventDestroy(ev0); if(ev1) hipEventDestroy(ev1); if(ev_w) hipEventDestroy(ev_w);
        if(st) hipStreamDestroy(st);
    }
};

namespace {

// The merge path: incoming items B (sorted, already matched against the resident set: match / ins / unm) into the other buffer set,
// which becomes the resident one.  Nothing of the resident set changes before the swap.
template<class In> int merge_path(ald_tset_dev *s, In B, const int64_t *match, const int64_t *ins, const int32_t *unm)
{
    hipStream_t st = s->st;
    SetBufs &Ab = s->res(), &Ob = s->buf[s->cur ^ 1];
    const SetView A = Ab.view(); const int64_t nA = Ab.n, nB = B.n;
    MergeScratch &M = s->mg;
    DevBuf &d_ub = M.ub, &d_cnt = M.cnt, &d_shift = M.shift, &d_rmatch = M.rmatch, &d_slot = M.slot, &d_ecnt = M.ecnt, &d_scnt = M.scnt, &d_tmp = M.cub_tmp;
    if(d_ub.ensure(4 * (size_t)(nB + 1)) || d_cnt.ensure(4 * (size_t)(nA + 1)) || d_shift.ensure(4 * (size_t)(nA + 1)) || d_rmatch.ensure(8 * (size_t)(nA + 1))) return ald_set_err(ALD_ERR_NOMEM, "resident set merge scratch");
    const char *const scan = "resident set scan scratch";
    { int rc = tx_cub(d_tmp, scan, [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int32_t*)unm, (int32_t*)d_ub.p, (int)(nB + 1), st); }); if(rc != ALD_OK) return rc; }
    HCHK(hipMemsetAsync(d_cnt.p, 0, 4 * (size_t)(nA + 1), st));
    HCHK(hipMemsetAsync(d_rmatch.p, 0xFF, 8 * (size_t)(nA + 1), st));
    if(nB > 0) hipLaunchKernelGGL(rs_mark, dim3(grid_for(nB)), dim3(TX_BLOCK), 0, st, match, ins, nB, (int64_t*)d_rmatch.p, (int32_t*)d_cnt.p);
    { int rc = tx_cub(d_tmp, scan, [&](void *t, size_t &nb) { return hipcub::DeviceScan::InclusiveSum(t, nb, (const int32_t*)d_cnt.p, (int32_t*)d_shift.p, (int)(nA + 1), st); }); if(rc != ALD_OK) return rc; }
    PinBuf &p_cnt = s->tx.p_count;
    if(p_cnt.ensure(64)) return ald_set_err(ALD_ERR_NOMEM, "pinned counter");
    int64_t *hc = (int64_t*)p_cnt.p;
    { int32_t *u = (int32_t*)(hc + 4); HCHK(hipMemcpyAsync(u, (const int32_t*)d_ub.p + nB, 4, hipMemcpyDeviceToHost, st)); HCHK(hipStreamSynchronize(st)); hc[0] = *u; }
    s->bytes_to_host += 4 + 16;                             // (this count and the two totals below)
    const int64_t N = nA + hc[0];
    if(d_slot.ensure(8 * (size_t)(N + 1)) || d_ecnt.ensure(8 * (size_t)(N + 1)) || d_scnt.ensure(8 * (size_t)(N + 1)) || Ob.ensure_items(N)) return ald_set_err(ALD_ERR_NOMEM, "resident set items");
    if(N > 0) hipLaunchKernelGGL(rs_slots, dim3(grid_for(nA + nB)), dim3(TX_BLOCK), 0, st, nA, nB, (const int32_t*)d_shift.p, match, ins, (const int32_t*)d_ub.p, (int64_t*)d_slot.p);
    hipLaunchKernelGGL(rs_sizes<In>, dim3(grid_for(N + 1)), dim3(TX_BLOCK), 0, st, A, B, (const int64_t*)d_slot.p, (const int64_t*)d_rmatch.p, N, (int64_t*)d_ecnt.p, (int64_t*)d_scnt.p);
    { int rc = tx_cub(d_tmp, scan, [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int64_t*)d_ecnt.p, (int64_t*)Ob.eoff.p, (int)(N + 1), st); }); if(rc != ALD_OK) return rc; }
    { int rc = tx_cub(d_tmp, scan, [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int64_t*)d_scnt.p, (int64_t*)Ob.soff.p, (int)(N + 1), st); }); if(rc != ALD_OK) return rc; }
    HCHK(hipMemcpyAsync(hc + 1, (const int64_t*)Ob.eoff.p + N, 8, hipMemcpyDeviceToHost, st));
    HCHK(hipMemcpyAsync(hc + 2, (const int64_t*)Ob.soff.p + N, 8, hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    const int64_t NE = hc[1], NS = hc[2];
    if(Ob.ensure_tail(NE, NS)) return ald_set_err(ALD_ERR_NOMEM, "resident set exons / samples");
    Ob.n = N; Ob.ne = NE; Ob.ns = NS;
    const SetView O = Ob.view();
    if(N > 0) hipLaunchKernelGGL(rs_write<In>, dim3(grid_for(N)), dim3(TX_BLOCK), 0, st, A, B, (const int64_t*)d_slot.p, (const int64_t*)d_rmatch.p, N, O);
    if(s->ev1) HCHK(hipEventRecord(s->ev1, st));
    HCHK(hipStreamSynchronize(st));
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a resident-set kernel failed");
    s->cur ^= 1;
    return ALD_OK;
}

// One batch (or stream) of records into the set.  d_pool / d_roff: records in (graph, path) order on the device; h_pool / h_roff / h_cov:
// the same on the host (the single-exon part is merged there); label / h_tid as in tset_reduce.hip's reduce_core.
// h_pool = null (a batch that ald_batch_finish ended: its records never left HBM): the two things the host part needs are fetched here --
// the weights, 8 bytes per path, for coverage = log(1 + weight) with the host's libm, under the sort; and, unless skip_single_exon, the
// records of the transcripts with fewer than two exons, compacted on the device.
// d_cov / d_tid (a device stream folded with the caller's coverage[] / tid[], h_pool = null): the same per path in DEVICE memory -- the
// weights then stay where they are; h_cov / h_tid are only read for the transcripts the host part merges.
int add_records(ald_tset_dev *s, const uint32_t *d_pool, const unsigned long long *d_roff, const uint32_t *h_pool, const unsigned long long *h_roff, const double *h_cov,
                const int64_t *h_tid, int64_t np, int n_graphs, const int32_t *sid, const int64_t *label, int64_t tid_base, int32_t skip_single_exon,
                const double *d_cov = nullptr, const int64_t *d_tid = nullptr)
{
    s->last_device_ms = 0;
    if(np == 0) return ALD_OK;
    hipStream_t st = s->st;
    RedScratch S; S.x = &s->tx; S.st = st; S.d2h = &s->bytes_to_host;
    TxIn in; in.roff = d_roff; in.pool = d_pool; in.np = np;
    TxFront X; X.ev0 = s->ev0;
    const unsigned long long *h_off = nullptr;             // != null: h_pool holds the single-exon records only, in the order of X.host_paths
    if(h_pool) { int rc = tx_front_groups(S, in, h_cov, n_graphs, sid, X); if(rc != ALD_OK) return rc; }
    else {
        X.ev_w = s->ev_w; X.d_cov = d_cov;
        { int rc = tx_front_sort(S, in, nullptr, n_graphs, sid, X); if(rc != ALD_OK) return rc; }
        if(!d_cov) { int rc = tx_front_coverage(S, X); if(rc != ALD_OK) return rc; }
        { int rc = tx_front_heads(S, in, X); if(rc != ALD_OK) return rc; }
        if(!d_cov) h_cov = X.h_cov;
        h_roff = nullptr;
        if(!skip_single_exon) { int rc = tx_compact_singles(S, in, X, s->mg.singles, &h_pool, &h_off); if(rc != ALD_OK) return rc; }      // read behind the stream waits below
    }
    if(X.n_groups > 0) {
        const int64_t G = X.n_groups;
        MergeScratch &M = s->mg;
        DevBuf &d_ghead = M.ghead, &d_perm = M.perm, &d_match = M.match, &d_ins = M.ins, &d_unm = M.unm, &d_start = M.start, &d_sbeg = M.sbeg, &d_lab = s->d_label, &d_ptid = s->d_tid;
        if(d_ghead.ensure(4 * (size_t)G) || d_perm.ensure(4 * (size_t)G) || d_match.ensure(8 * (size_t)G) || d_ins.ensure(8 * (size_t)G) || d_unm.ensure(4 * (size_t)(G + 1))
           || d_start.ensure(8 * (size_t)G) || d_sbeg.ensure(8 * (size_t)(G + 1)) || (label && d_lab.ensure(8 * (size_t)n_graphs + 8)) || (h_tid && !d_tid && d_ptid.ensure(8 * (size_t)np + 8)))
            return ald_set_err(ALD_ERR_NOMEM, "resident set batch scratch");
        if(label) HCHK(hipMemcpyAsync(d_lab.p, label, 8 * (size_t)n_graphs, hipMemcpyHostToDevice, st));
        if(h_tid && !d_tid) HCHK(hipMemcpyAsync(d_ptid.p, h_tid, 8 * (size_t)np, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(rs_ghead, dim3(grid_for(X.n_dev)), dim3(TX_BLOCK), 0, st, tx_head(S), tx_gid(S), X.n_dev, (int32_t*)d_ghead.p);
        hipLaunchKernelGGL(rs_order, dim3(grid_for(G)), dim3(TX_BLOCK), 0, st, in, tx_sidx(S), (const int32_t*)d_ghead.p, tx_skey(S), G, (int32_t*)d_perm.p);
        InBatch B; B.in = in; B.sidx = tx_sidx(S); B.ghead = (const int32_t*)d_ghead.p; B.skey = tx_skey(S); B.perm = (const int32_t*)d_perm.p;
        B.grp = nullptr; B.smp = nullptr; B.sbeg = nullptr; B.tid_base = tid_base; B.label = label ? (const int64_t*)d_lab.p : nullptr; B.ptid = d_tid ? d_tid : h_tid ? (const int64_t*)d_ptid.p : nullptr; B.n = G;
        const SetView A = s->res().view();
        hipLaunchKernelGGL(rs_match<InBatch>, dim3(grid_for(G + 1)), dim3(TX_BLOCK), 0, st, A, B, (int64_t*)d_match.p, (int64_t*)d_ins.p, (int32_t*)d_unm.p);
        hipLaunchKernelGGL(rs_start, dim3(grid_for(G)), dim3(TX_BLOCK), 0, st, (const int32_t*)d_perm.p, (const int64_t*)d_match.p, G, (int64_t*)d_start.p);
        { int rc = tx_front_fold(S, in, X, (const int64_t*)d_start.p, A.cov); if(rc != ALD_OK) return rc; }
        hipLaunchKernelGGL(rs_sbeg, dim3(grid_for(G + 1)), dim3(TX_BLOCK), 0, st, (const TxSample*)tx_samples(S), (int64_t)X.n_runs, G, (int64_t*)d_sbeg.p);
        B.grp = tx_groups(S); B.smp = tx_samples(S); B.sbeg = (const int64_t*)d_sbeg.p;
        { int rc = merge_path(s, B, (const int64_t*)d_match.p, (const int64_t*)d_ins.p, (const int32_t*)d_unm.p); if(rc != ALD_OK) return rc; }
    } else {
        HCHK(hipEventRecord(s->ev1, st));
        HCHK(hipStreamSynchronize(st));
    }
    float ms = 0; if(hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) s->last_device_ms = ms;
    // the device part is in: the transcripts with fewer than two exons, graph by graph, into the host part
    if(!skip_single_exon) tx_host_singles(s->single, X.host_paths, h_pool, h_roff, h_cov, h_tid, sid, label, tid_base, h_off);
    return ALD_OK;
}

// A stream in device memory: index, record build, fold -- nothing proportional to n_words leaves HBM.  coverage / tid: the caller's (host
// memory, one per transcript of the stream, left-out ones counted) or null.  A refused stream returns before anything of the set changes.
int add_device_stream(ald_tset_dev *s, const uint32_t *d_words, int64_t n_words, const double *coverage, const int64_t *tid, int64_t graph_offset, int64_t tid_base, int32_t skip_single_exon)
{
    hipStream_t st = s->st;
    StreamIndex I;
    { const int rc = tx_stream_index(st, s->ix, s->ev_i0, s->ev_i1, d_words, n_words, graph_offset, I);
      s->bytes_to_host += 40; s->st_index_ms = I.ms;
      if(rc != ALD_OK) return rc; }
    const int64_t nt = I.nt, ng = I.ng;
    s->st_transcripts = nt; s->st_groups = ng;
    StreamRecScratch &R = s->sr;
    DevBuf &d_len = R.len, &d_at = R.at, &d_keep = R.keep, &d_kord = R.kord, &d_tmp = R.cub_tmp, &d_covin = R.cov_in, &d_tidin = R.tid_in, &d_cov = R.cov, &d_tidk = R.tid;
    // a scratch record has 6 words more than its transcript has in the stream (ALD_REC_HDR + 2 + k against ALD_TS_HDR + k)
    if(d_len.ensure(8 * (size_t)(nt + 1)) || d_at.ensure(8 * (size_t)(nt + 1)) || d_keep.ensure(4 * (size_t)(nt + 1)) || d_kord.ensure(4 * (size_t)(nt + 1))
       || (coverage && (d_covin.ensure(8 * (size_t)nt) || d_cov.ensure(8 * (size_t)nt))) || (tid && (d_tidin.ensure(8 * (size_t)nt) || d_tidk.ensure(8 * (size_t)nt)))
       || s->d_pool.ensure(4 * (size_t)(n_words + (ALD_REC_HDR + 2 - ALD_TS_HDR) * nt) + 64) || s->d_roff.ensure(8 * (size_t)nt + 8) || R.p_head.ensure(16 + 12 * (size_t)ng + 64)) return ald_set_err(ALD_ERR_NOMEM, "resident set stream buffers");
    if(coverage) HCHK(hipMemcpyAsync(d_covin.p, coverage, 8 * (size_t)nt, hipMemcpyHostToDevice, st));
    if(tid) HCHK(hipMemcpyAsync(d_tidin.p, tid, 8 * (size_t)nt, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sr_len, dim3(grid_for(nt + 1)), dim3(TX_BLOCK), 0, st, d_words, I.toff, nt, (int)(skip_single_exon != 0), (int64_t*)d_len.p, (int32_t*)d_keep.p);
    { int rc = tx_cub(d_tmp, "scan scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int64_t*)d_len.p, (int64_t*)d_at.p, (int)(nt + 1), st); }); if(rc != ALD_OK) return rc; }
    { int rc = tx_cub(d_tmp, "scan scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int32_t*)d_keep.p, (int32_t*)d_kord.p, (int)(nt + 1), st); }); if(rc != ALD_OK) return rc; }
    hipLaunchKernelGGL(sr_emit, dim3(grid_for(16 * nt)), dim3(TX_BLOCK), 0, st, d_words, I.toff, I.gid, (const int64_t*)d_at.p, (const int32_t*)d_kord.p, nt,
                       coverage ? (const double*)d_covin.p : (const double*)nullptr, tid ? (const int64_t*)d_tidin.p : (const int64_t*)nullptr,
                       (uint32_t*)s->d_pool.p, (unsigned long long*)s->d_roff.p, (double*)d_cov.p, (int64_t*)d_tidk.p);
    // to the host: the number of kept transcripts, label + sid of every group (12 bytes per group)
    char *hp = (char*)R.p_head.p; int64_t *h_label = (int64_t*)(hp + 16); int32_t *h_sid = (int32_t*)(hp + 16 + 8 * (size_t)ng);
    HCHK(hipMemcpyAsync(hp, (const int32_t*)d_kord.p + nt, 4, hipMemcpyDeviceToHost, st));
    HCHK(hipMemcpyAsync(h_label, I.label, 8 * (size_t)ng, hipMemcpyDeviceToHost, st));
    HCHK(hipMemcpyAsync(h_sid, I.sid, 4 * (size_t)ng, hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "a stream-record kernel failed to launch");
    s->bytes_to_host += 4 + 12 * ng;
    const int64_t np = (int64_t)*(const int32_t*)hp;
    // without the filter every transcript is kept and a path's ordinal is its ordinal in the stream: coverage[] / tid[] serve the host part as they are
    return add_records(s, (const uint32_t*)s->d_pool.p, (const unsigned long long*)s->d_roff.p, nullptr, nullptr, coverage, tid, np, (int)ng, h_sid, h_label, tid_base, skip_single_exon,
                       coverage ? (const double*)d_cov.p : (const double*)nullptr, tid ? (const int64_t*)d_tidk.p : (const int64_t*)nullptr);
}

// The device part, copied back: flat arrays in the set's order (exon / sample offsets included), count2 = #samples
int fetch_device_part(const ald_tset_dev *s, ald_tset_flat &D)
{
    const FlatView R = s->res().flat();
    flat_resize(D, R.n, R.ne, R.ns);
    if(R.n == 0) return ALD_OK;
    hipError_t e = hipSuccess;
    for_each_column([&](FlatKind k, auto *dst, auto *src) { if(src && R.len(k) && e == hipSuccess) e = hipMemcpyAsync(dst, src, sizeof(*src) * R.len(k), hipMemcpyDeviceToHost, s->st); }, flat_mut(D), R);
    if(e != hipSuccess) return ald_set_err(ALD_ERR_HIP, std::string("resident set, device to host: ") + hipGetErrorString(e));
    HCHK(hipStreamSynchronize(s->st));
    for(int64_t i = 0; i < R.n; i++) D.count2[(size_t)i] = (int32_t)(D.sample_offset[(size_t)i + 1] - D.sample_offset[(size_t)i]);
    return ALD_OK;
}

// the whole set, flat, in the reference's iteration order: the host items (fewer than two exons) spliced in by hash, ahead of the device
// items of the same hash (compare1 puts fewer exons first, transcript.cc:271)
int snapshot(const ald_tset_dev *s, ald_tset_flat &F)
{
    ald_tset_flat D;
    { int rc = fetch_device_part(s, D); if(rc != ALD_OK) return rc; }
    const SinkRows H = sink_rows(&s->single, 1);
    const FlatView Dv = flat_view(D); const int64_t NG = Dv.n, NH = (int64_t)H.item.size();
    if(NH == 0) F = std::move(D);
    else {
        flat_resize(F, NG + NH, Dv.ne + H.ne, Dv.ns + H.ns);
        const FlatMut Fv = flat_mut(F); int64_t k = 0;
        for(const auto &at : merge_order({HashRun{H.hash.data(), NH}, HashRun{Dv.hash, NG}}))
            if(at.first == 0) flat_put_item(Fv, k++, H.hash[(size_t)at.second], *H.item[(size_t)at.second]); else flat_copy_row(Fv, k++, Dv, at.second);
    }
    F.n_device_groups = NG; F.n_host_items = NH;
    return ALD_OK;
}

} // namespace

extern "C" {

int ald_tset_dev_create(int32_t device, double single_exon_overlap, ald_tset_dev **out)
{
    if(!out) return ALD_ERR_INVALID;
    *out = nullptr;
    { int rc = tx_need_device(device, "the resident transcript set"); if(rc != ALD_OK) return rc; }
    HCHK(hipSetDevice(device));
    std::unique_ptr<ald_tset_dev> s(new ald_tset_dev(single_exon_overlap));
    s->device = device;
    HCHK(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
    HCHK(hipEventCreate(&s->ev0)); HCHK(hipEventCreate(&s->ev1)); HCHK(hipEventCreateWithFlags(&s->ev_w, hipEventDisableTiming));
    HCHK(hipEventCreate(&s->ev_i0)); HCHK(hipEventCreate(&s->ev_i1));
    *out = s.release();
    return ALD_OK;
}

int ald_tset_dev_destroy(ald_tset_dev *s)
{
    if(!s) return ALD_OK;
    hipSetDevice(s->device);
    if(s->st) hipStreamSynchronize(s->st);
    delete s;
    return ALD_OK;
}

int ald_tset_dev_add_batch(ald_tset_dev *s, const ald_batch *cb, const int32_t *sid, int64_t tid_base, int32_t skip_single_exon)
{
    if(!s || !cb) return ALD_ERR_INVALID;
    if(cb->device != s->device) return ald_set_err(ALD_ERR_INVALID, "ald_tset_dev_add_batch: the batch lives on another device");
    if(!cb->downloaded && !cb->finished) return ald_set_err(ALD_ERR_STATE, "ald_tset_dev_add_batch before ald_batch_download / ald_batch_finish");
    const auto T0 = std::chrono::steady_clock::now();
    ald_batch *b = const_cast<ald_batch*>(cb);
    HCHK(hipSetDevice(s->device));
    { int rc = device_path_table(b); if(rc != ALD_OK) return rc; }
    HCHK(hipStreamSynchronize(b->stream));                 // the path table is built on the batch's stream; everything else runs on the set's
    const bool host = b->downloaded;                        // a batch that is only finished has no host copy of its records
    const int rc = add_records(s, (const uint32_t*)b->d_pool.p, (const unsigned long long*)b->d_ordoff.p, host ? b->res.pool_data() : nullptr, host ? (const unsigned long long*)b->res.rec_off.data() : nullptr,
                               host ? b->res.coverage.data() : nullptr, nullptr, b->total_paths, b->hb.n(), sid, nullptr, tid_base, skip_single_exon);
    s->last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    return rc;
}

int ald_tset_dev_add_stream(ald_tset_dev *s, const uint32_t *words, int64_t n_words, const double *coverage, const int64_t *tid, int32_t graph_offset, int64_t tid_base, int32_t skip_single_exon)
{
    if(!s || n_words < 0 || (n_words > 0 && !words)) return ALD_ERR_INVALID;
    const auto T0 = std::chrono::steady_clock::now();
    HCHK(hipSetDevice(s->device));
    s->st_transcripts = s->st_groups = s->st_words_to_host = s->bytes_to_host = 0; s->st_index_ms = 0;
    const bool dev = n_words > 0 && tx_on_device(words);
    if(dev && n_words < (int64_t)1 << 31) {                 // a stream in device memory (e.g. a segment the owner exchange left there) stays there
        const int rc = add_device_stream(s, words, n_words, coverage, tid, graph_offset, tid_base, skip_single_exon);
        s->last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
        return rc;
    }
    std::vector<uint32_t> staged;                           // 2^31 words or more: beyond the index's 32-bit nodes, it comes to the host for the walk
    if(dev) {
        staged.resize((size_t)n_words);
        HCHK(hipMemcpy(staged.data(), words, 4 * (size_t)n_words, hipMemcpyDeviceToHost));
        words = staged.data(); s->st_words_to_host = n_words; s->bytes_to_host += 4 * n_words;
    }
    StreamRecords R;
    { int rc = tx_stream_records(words, n_words, coverage, tid, skip_single_exon, graph_offset, R); if(rc != ALD_OK) return rc; }
    s->st_transcripts = R.n_transcripts; s->st_groups = (int64_t)R.label.size();
    const int64_t np = (int64_t)R.roff.size();
    if(np > 0) {
        if(s->d_pool.ensure(4 * R.pool.size() + 64) || s->d_roff.ensure(8 * (size_t)np + 8)) return ald_set_err(ALD_ERR_NOMEM, "resident set stream buffers");
        HCHK(hipMemcpyAsync(s->d_pool.p, R.pool.data(), 4 * R.pool.size(), hipMemcpyHostToDevice, s->st));
        HCHK(hipMemcpyAsync(s->d_roff.p, R.roff.data(), 8 * (size_t)np, hipMemcpyHostToDevice, s->st));
    }
    const int rc = add_records(s, (const uint32_t*)s->d_pool.p, (const unsigned long long*)s->d_roff.p, R.pool.data(), R.roff.data(), R.cov.data(), tid ? R.tids.data() : nullptr,
                               np, (int)R.label.size(), R.sid.empty() ? nullptr : R.sid.data(), R.label.data(), tid_base, 0 /* filtered above */);
    s->last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    return rc;
}

int ald_tset_dev_stream_stats(const ald_tset_dev *s, int64_t *n_transcripts, int64_t *n_graphs, int64_t *words_to_host, int64_t *bytes_to_host, double *index_ms)
{
    if(!s) return ALD_ERR_INVALID;
    if(n_transcripts) *n_transcripts = s->st_transcripts; if(n_graphs) *n_graphs = s->st_groups;
    if(words_to_host) *words_to_host = s->st_words_to_host; if(bytes_to_host) *bytes_to_host = s->bytes_to_host;
    if(index_ms) *index_ms = s->st_index_ms;
    return ALD_OK;
}

int ald_tset_dev_merge(ald_tset_dev *dst, ald_tset_dev *src)
{
    if(!dst || !src || dst == src) return ALD_ERR_INVALID;
    if(dst->device != src->device) return ald_set_err(ALD_ERR_INVALID, "ald_tset_dev_merge: the sets live on different devices");
    const auto T0 = std::chrono::steady_clock::now();
    HCHK(hipSetDevice(dst->device));
    HCHK(hipStreamSynchronize(src->st));
    SetBufs &Sb = src->res(); const int64_t nB = Sb.n;
    dst->last_device_ms = 0;
    if(nB > 0) {
        hipStream_t st = dst->st;
        DevBuf &d_match = dst->mg.match, &d_ins = dst->mg.ins, &d_unm = dst->mg.unm;
        if(d_match.ensure(8 * (size_t)nB) || d_ins.ensure(8 * (size_t)nB) || d_unm.ensure(4 * (size_t)(nB + 1))) return ald_set_err(ALD_ERR_NOMEM, "resident set merge scratch");
        HCHK(hipEventRecord(dst->ev0, st));
        InSet B; B.v = Sb.view(); B.n = nB;
        hipLaunchKernelGGL(rs_match<InSet>, dim3(grid_for(nB + 1)), dim3(TX_BLOCK), 0, st, dst->res().view(), B, (int64_t*)d_match.p, (int64_t*)d_ins.p, (int32_t*)d_unm.p);
        { int rc = merge_path(dst, B, (const int64_t*)d_match.p, (const int64_t*)d_ins.p, (const int32_t*)d_unm.p); if(rc != ALD_OK) return rc; }
        float ms = 0; if(hipEventElapsedTime(&ms, dst->ev0, dst->ev1) == hipSuccess) dst->last_device_ms = ms;
    }
    dst->single.add(src->single);                           // transcript_set::add(transcript_set&) for the host part
    src->single.clear(); Sb.n = Sb.ne = Sb.ns = 0;
    dst->last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    return ALD_OK;
}

int ald_tset_dev_size(const ald_tset_dev *s, int64_t *n_items, int64_t *n_exons, int64_t *n_samples)
{
    if(!s) return ALD_ERR_INVALID;
    int64_t a = s->res().n, e = s->res().ne, m = s->res().ns;
    for(auto &x : s->single.mt) for(auto &z : x.second) { a++; e += (int64_t)z.trst.n_exons(); m += (int64_t)z.samples.size(); }
    if(n_items) *n_items = a; if(n_exons) *n_exons = e; if(n_samples) *n_samples = m;
    return ALD_OK;
}

int ald_tset_dev_snapshot(const ald_tset_dev *s, ald_tset_flat **out)
{
    if(!s || !out) return ALD_ERR_INVALID;
    const auto T0 = std::chrono::steady_clock::now();
    HCHK(hipSetDevice(s->device));
    std::unique_ptr<ald_tset_flat> F(new ald_tset_flat());
    { int rc = snapshot(s, *F); if(rc != ALD_OK) return rc; }
    F->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    *out = F.release();
    return ALD_OK;
}

int ald_tset_dev_export(const ald_tset_dev *s, uint64_t *hash, int32_t *count, char *strand, double *coverage, double *cov2, double *conf, double *abd,
                        int32_t *count1, int32_t *count2, int64_t *tid, int64_t *exon_offset, int32_t *exon_lr,
                        int64_t *sample_offset, int32_t *sample_sid, double *sample_cov2, double *sample_conf, double *sample_abd, int32_t *sample_count1)
{
    if(!s) return ALD_ERR_INVALID;
    ald_tset_flat *F = nullptr;
    { int rc = ald_tset_dev_snapshot(s, &F); if(rc != ALD_OK) return rc; }
    const int rc = ald_tset_flat_export(F, hash, count, strand, coverage, cov2, conf, abd, count1, count2, tid, exon_offset, exon_lr, sample_offset, sample_sid, sample_cov2, sample_conf, sample_abd, sample_count1);
    ald_tset_flat_free(F);
    return rc;
}

int ald_tset_dev_stats(const ald_tset_dev *s, double *last_device_ms, double *last_call_ms, int64_t *device_items, int64_t *host_items)
{
    if(!s) return ALD_ERR_INVALID;
    if(last_device_ms) *last_device_ms = s->last_device_ms; if(last_call_ms) *last_call_ms = s->last_call_ms;
    if(device_items) *device_items = s->res().n;
    if(host_items) *host_items = (int64_t)s->single.size();
    return ALD_OK;
}

} // extern "C"
