// tset_partition.hip -- the finished transcripts of a batch, or an existing transcript stream, split by BUCKET OWNER for a world of W ranks.
//
// transcript_set is a map from transcript::get_intron_chain_hashing to a bucket, and transcript_set::add / merge_sorted_trans_items only
// ever touch one bucket at a time (rnacore/transcript_set.cc:83-120, 149-175; gtf/transcript.cc:183-201) -- single-exon transcripts
// included, whose key is their mid-point bin.  So the rank that owns bucket h, h % W, computes that bucket bit for bit as an unsharded
// run would, provided it receives the bucket's transcripts in ascending global (graph, path) order.  The kernels here make W sub-streams,
// back to back in one device buffer, sub-stream r holding exactly the transcripts with hash % W == r in their original order, in the
// unchanged record format of ald_batch_transcript_stream; ald_comm_exchange_streams (comm_rccl.cpp) then sends sub-stream r to rank r.
//
// Kernels (streaming, HBM-bound passes; the sort is a hipCUB radix sort over ceil(log2 W) bits, stable, so the order inside an owner stays):
//   tp_owner    1 lane / transcript      bucket hash -> owner, record length
//   tp_gather   1 lane / sorted place    length of the transcript that lands there (then an exclusive scan: where it lands)
//   tp_bounds   1 lane / sorted place    where the owner changes: offsets[owner]
//   tp_emit     16 lanes / transcript    header + exon words, consecutive lanes on consecutive words (as ts_emit)
// Both sources go through the same kernels: REC = the path records of a batch (exon join and header layout of ts_emit, no unsplit stream
// is built first), !REC = the transcripts of a stream at the word offsets the stream index found (tset_index.hip: kernels, not a host walk).
#include "tset_front.h"
#include <hipcub/hipcub.hpp>

namespace {

// transcript p lies at base + off[p]: a path record (REC) or a stream record
struct TpSrc { const uint32_t *base; const unsigned long long *off; int64_t n; };

template<bool REC> __global__ void tp_owner(TpSrc s, int skip_single, uint32_t world, uint32_t *owner, int32_t *ord, int32_t *len)
{
    const int64_t p = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(p >= s.n) return;
    const uint32_t *r = s.base + s.off[p];
    const int k = REC ? (int)r[ALD_REC_NEXW] : 2 * (int)r[ALD_TS_NEXONS];
    const int32_t *ex = REC ? rec_exons(r) : ts_exons(r);
    owner[p] = (uint32_t)(bucket_key_dev(ex, k) % world);
    ord[p] = (int32_t)p;
    len[p] = (k <= 2 && skip_single) ? 0 : ALD_TS_HDR + k;
}
__global__ void tp_gather(const int32_t *sord, const int32_t *len, int64_t n, int64_t *slen)
{
    const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(i > n) return;
    slen[i] = i < n ? (int64_t)len[sord[i]] : 0;          // (the exclusive scan over n + 1 entries leaves the total in the last one)
}
// offsets[r] = first word of owner r's sub-stream, offsets[world] = the total: place i sets the owners that begin between its predecessor and itself
__global__ void tp_bounds(const uint32_t *sown, const int64_t *at, int64_t n, int world, int64_t *offsets)
{
    const int64_t i = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if(i > n) return;
    const int lo = i == 0 ? 0 : (int)sown[i - 1] + 1, hi = i == n ? world : (int)sown[i];
    for(int r = lo; r <= hi; r++) offsets[r] = at[i];
}
template<bool REC> __global__ void tp_emit(TpSrc s, const int32_t *sord, const int64_t *at, const int32_t *sid, uint32_t *out)
{
    const int64_t i = ((int64_t)blockIdx.x * TX_BLOCK + threadIdx.x) / 16; const int l = (int)(threadIdx.x & 15);
    if(i >= s.n) return;
    const int64_t o = at[i], n = at[i + 1] - o;
    if(n == 0) return;
    const uint32_t *r = s.base + s.off[sord[i]];
    uint32_t *w = out + o;
    if(!REC) { for(int64_t q = l; q < n; q += 16) w[q] = r[q]; return; }
    const int k = (int)r[ALD_REC_NEXW];
    if(l < ALD_TS_HDR) w[l] = ts_header_word(r, l, sid);
    const uint32_t *x = (const uint32_t*)rec_exons(r);
    for(int q = l; q < k; q += 16) w[ALD_TS_HDR + q] = x[q];
}

// owner, stable sort, placement; h_offsets[world + 1] is on the host on return
template<bool REC> int tp_place(hipStream_t st, OwnerSplitScratch &T, TpSrc s, int skip_single, int world, int64_t *h_offsets)
{
    const int64_t n = s.n;
    if(n >= (int64_t)1 << 31) return ald_set_err(ALD_ERR_INVALID, "owner split: more than 2^31 - 1 transcripts");
    if(T.owner.ensure(4 * (size_t)n) || T.owner_sorted.ensure(4 * (size_t)n) || T.ord.ensure(4 * (size_t)n) || T.ord_sorted.ensure(4 * (size_t)n) || T.len.ensure(4 * (size_t)n)
       || T.len_sorted.ensure(8 * (size_t)n + 8) || T.place.ensure(8 * (size_t)n + 8) || T.offsets.ensure(8 * (size_t)(world + 1))) return ald_set_err(ALD_ERR_NOMEM, "owner split buffers");
    int bits = 1; while((1 << bits) < world) bits++;
    hipLaunchKernelGGL(tp_owner<REC>, dim3(grid_for(n)), dim3(TX_BLOCK), 0, st, s, skip_single, (uint32_t)world, (uint32_t*)T.owner.p, (int32_t*)T.ord.p, (int32_t*)T.len.p);
    { int rc = tx_cub(T.cub_tmp, "owner split scratch", [&](void *t, size_t &nb) { return hipcub::DeviceRadixSort::SortPairs(t, nb, (const uint32_t*)T.owner.p, (uint32_t*)T.owner_sorted.p, (const int32_t*)T.ord.p, (int32_t*)T.ord_sorted.p, (int)n, 0, bits, st); }); if(rc != ALD_OK) return rc; }
    hipLaunchKernelGGL(tp_gather, dim3(grid_for(n + 1)), dim3(TX_BLOCK), 0, st, (const int32_t*)T.ord_sorted.p, (const int32_t*)T.len.p, n, (int64_t*)T.len_sorted.p);
    { int rc = tx_cub(T.cub_tmp, "owner split scratch", [&](void *t, size_t &nb) { return hipcub::DeviceScan::ExclusiveSum(t, nb, (const int64_t*)T.len_sorted.p, (int64_t*)T.place.p, (int)(n + 1), st); }); if(rc != ALD_OK) return rc; }
    hipLaunchKernelGGL(tp_bounds, dim3(grid_for(n + 1)), dim3(TX_BLOCK), 0, st, (const uint32_t*)T.owner_sorted.p, (const int64_t*)T.place.p, n, world, (int64_t*)T.offsets.p);
    HCHK(hipMemcpyAsync(h_offsets, T.offsets.p, 8 * (size_t)(world + 1), hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "an owner-split kernel failed to launch");
    return ALD_OK;
}
template<bool REC> int tp_fill(hipStream_t st, OwnerSplitScratch &T, TpSrc s, const int32_t *d_sid, uint32_t *d_out)
{
    hipLaunchKernelGGL(tp_emit<REC>, dim3(grid_for(16 * s.n)), dim3(TX_BLOCK), 0, st, s, (const int32_t*)T.ord_sorted.p, (const int64_t*)T.place.p, d_sid, d_out);
    HCHK(hipStreamSynchronize(st));
    if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "an owner-split kernel failed to launch");
    return ALD_OK;
}

} // namespace

extern "C" {

int ald_transcript_bucket(const int32_t *exon_lr, int32_t n_exons, uint64_t *hash)
{
    if(!hash || n_exons < 0 || (n_exons > 0 && !exon_lr)) return ALD_ERR_INVALID;
    *hash = bucket_key_dev(exon_lr, 2 * (int)n_exons);
    return ALD_OK;
}

int ald_batch_device_transcript_streams_by_owner(const ald_batch *cb, const int32_t *sid, int32_t skip_single_exon, int32_t world, void **dev_words, const int64_t **offsets)
{
    if(!cb || !dev_words || !offsets) return ALD_ERR_INVALID;
    if(world < 1 || world > 64) return ald_set_err(ALD_ERR_INVALID, "owner split: world must be in 1..64");
    if(!cb->downloaded && !cb->finished) return ald_set_err(ALD_ERR_STATE, "ald_batch_device_transcript_streams_by_owner before ald_batch_download / ald_batch_finish");
    ald_batch *b = const_cast<ald_batch*>(cb);
    HCHK(hipSetDevice(b->device));
    const int n = b->hb.n(); const int64_t np = b->total_paths;
    b->tp_offsets.assign((size_t)world + 1, 0);
    *dev_words = nullptr; *offsets = b->tp_offsets.data();
    if(np == 0) return ALD_OK;
    { int rc = device_path_table(b); if(rc != ALD_OK) return rc; }
    DevBuf &d_sid = b->tx.sid, &d_out = b->tp.out;
    hipStream_t st = b->stream;
    if(sid) { if(d_sid.ensure(4 * (size_t)n + 4)) return ald_set_err(ALD_ERR_NOMEM, "transcript stream buffers"); HCHK(hipMemcpyAsync(d_sid.p, sid, 4 * (size_t)n, hipMemcpyHostToDevice, st)); }
    TpSrc s; s.base = (const uint32_t*)b->d_pool.p; s.off = (const unsigned long long*)b->d_ordoff.p; s.n = np;
    { int rc = tp_place<true>(st, b->tp, s, (int)(skip_single_exon != 0), world, b->tp_offsets.data()); if(rc != ALD_OK) return rc; }
    const int64_t total = b->tp_offsets[(size_t)world];
    if(total < 0 || d_out.ensure(4 * (size_t)total + 64)) return ald_set_err(ALD_ERR_NOMEM, "transcript streams by owner");
    { int rc = tp_fill<true>(st, b->tp, s, sid ? (const int32_t*)d_sid.p : (const int32_t*)nullptr, (uint32_t*)d_out.p); if(rc != ALD_OK) return rc; }
    *dev_words = d_out.p;
    return ALD_OK;
}

int ald_tset_split_stream(int32_t device, const uint32_t *words, int64_t n_words, int32_t world, uint32_t *out_words, int64_t *offsets)
{
    if(!offsets || n_words < 0 || (n_words > 0 && (!words || !out_words))) return ALD_ERR_INVALID;
    if(world < 1 || world > 64) return ald_set_err(ALD_ERR_INVALID, "owner split: world must be in 1..64");
    { int rc = tx_need_device(device, "the owner split"); if(rc != ALD_OK) return rc; }
    HCHK(hipSetDevice(device));
    for(int r = 0; r <= world; r++) offsets[r] = 0;
    if(n_words == 0) return ALD_OK;
    const bool src_dev = tx_on_device(words), dst_dev = tx_on_device(out_words);
    Scoped<OwnerSplitScratch> tp; Scoped<StreamIndexScratch> ix; Scoped<DevBuf> d_in, d_off;
    DevBuf &d_out = tp.out;                                 // (only when the caller's buffer is on the host)
    ScopedStream stream; HCHK(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));
    hipStream_t st = stream.s;
    if((!src_dev && d_in.ensure(4 * (size_t)n_words)) || (!dst_dev && d_out.ensure(4 * (size_t)n_words))) return ald_set_err(ALD_ERR_NOMEM, "owner split buffers");
    TpSrc s; s.base = src_dev ? words : (const uint32_t*)d_in.p;
    if(n_words < (int64_t)1 << 31) {
        // the transcript boundaries come from the stream index: a device stream stays where it is, a host stream is uploaded once
        if(!src_dev) HCHK(hipMemcpyAsync(d_in.p, words, 4 * (size_t)n_words, hipMemcpyHostToDevice, st));
        StreamIndex I;
        { int rc = tx_stream_index(st, ix, nullptr, nullptr, s.base, n_words, 0, I); if(rc != ALD_OK) return rc; }
        s.off = I.toff; s.n = I.nt;
    } else {
        // 2^31 words or more, beyond the index's 32-bit nodes: the record walk on the host (as tx_stream_records walks); a device stream comes over for it
        std::vector<uint32_t> staged;
        const uint32_t *h_words = words;
        if(src_dev) { staged.resize((size_t)n_words); HCHK(hipMemcpy(staged.data(), words, 4 * (size_t)n_words, hipMemcpyDeviceToHost)); h_words = staged.data(); }
        std::vector<unsigned long long> toff;
        { int rc = tx_walk_stream(h_words, n_words, [&](int64_t o, bool) { toff.push_back((unsigned long long)o); }); if(rc != ALD_OK) return rc; }
        const int64_t nt = (int64_t)toff.size();
        if(d_off.ensure(8 * (size_t)nt)) return ald_set_err(ALD_ERR_NOMEM, "owner split buffers");
        if(!src_dev) HCHK(hipMemcpyAsync(d_in.p, words, 4 * (size_t)n_words, hipMemcpyHostToDevice, st));
        HCHK(hipMemcpy(d_off.p, toff.data(), 8 * (size_t)nt, hipMemcpyHostToDevice));
        s.off = (const unsigned long long*)d_off.p; s.n = nt;
    }
    std::vector<int64_t> h_offs((size_t)world + 1, 0);
    { int rc = tp_place<false>(st, tp, s, 0, world, h_offs.data()); if(rc != ALD_OK) return rc; }
    if(h_offs[(size_t)world] != n_words) return ald_set_err(ALD_ERR_HIP, "owner split: the sub-streams do not add up to the stream");
    uint32_t *d_dst = dst_dev ? out_words : (uint32_t*)d_out.p;
    { int rc = tp_fill<false>(st, tp, s, nullptr, d_dst); if(rc != ALD_OK) return rc; }
    if(!dst_dev) HCHK(hipMemcpy(out_words, d_dst, 4 * (size_t)n_words, hipMemcpyDeviceToHost));
    for(int r = 0; r <= world; r++) offsets[r] = h_offs[(size_t)r];
    return ALD_OK;
}

} // extern "C"
