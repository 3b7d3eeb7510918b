// comm_rccl.cpp -- the path's one exchange step for a MULTI-PROCESS host (one process per MI355X), behind the C ABI: every rank's
// finished-transcript stream (ald_batch_transcript_stream) travels to rank 0 over RCCL / xGMI, where ald_tset_add_stream merges the
// streams in rank order == ascending global graph id.  The analogue of the reference's `tm.add(ts)` under `mylock`
// (meta/assembler.cc:1127-1132), once per batch instead of once per graph.
//
// RCCL is loaded on first use (dlopen of librccl.so, RTLD_LOCAL): a host that runs all its devices in ONE process
// (aletsch::gpu_assembly_queue over a device list) never needs it, and a Python test process that already carries torch's own RCCL is
// not handed a second copy at load time.  Bootstrap is the caller's: rank 0 makes the 128-byte id (ald_comm_unique_id) and ships it
// to the other ranks by whatever it has (a file, a pipe, MPI, the reference's own thread pool has no such thing).
//
// Exchange = sizes by ncclAllGather (one int64 per rank), payloads by grouped ncclSend / ncclRecv to rank 0 -- point-to-point, which
// is what xGMI is; payload per rank is ~0.2 GB at 125 k graphs, i.e. ~1.4 ms per link.
//
// The funnel has a second form that leaves no rank with more than its share: ald_comm_exchange_streams sends sub-stream r of every rank
// (tset_partition.hip: the transcripts of the buckets rank r owns, hash % W == r) to rank r, all to all, where it folds into that rank's
// resident set; ald_comm_gather_sets then brings the W disjoint sets to rank 0, which interleaves them by hash.
#include "tset_front.h"          // ald_tset_flat (ald_comm_gather_sets), HCHK
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <mutex>
#include <memory>

namespace {

struct Rccl {
    void *h = nullptr; bool ok = false; std::string err;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl &rccl()
{
    static Rccl R; static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {getenv("ALD_RCCL_LIB"), "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for(const char *n : names) { if(!n) continue; R.h = dlopen(n, RTLD_NOW | RTLD_LOCAL); if(R.h) break; }
        if(!R.h) { R.err = std::string("librccl.so could not be loaded: ") + (dlerror() ? dlerror() : "?"); return; }
#define ALD_SYM(field, name) R.field = (decltype(R.field))dlsym(R.h, name); if(!R.field) { R.err = std::string("librccl.so lacks ") + name; return; }
        ALD_SYM(GetUniqueId, "ncclGetUniqueId") ALD_SYM(CommInitRank, "ncclCommInitRank") ALD_SYM(CommDestroy, "ncclCommDestroy") ALD_SYM(AllGather, "ncclAllGather")
        ALD_SYM(Send, "ncclSend") ALD_SYM(Recv, "ncclRecv") ALD_SYM(GroupStart, "ncclGroupStart") ALD_SYM(GroupEnd, "ncclGroupEnd") ALD_SYM(GetErrorString, "ncclGetErrorString")
#undef ALD_SYM
        R.ok = true;
    });
    return R;
}
#define NCHK(x) do { ncclResult_t r_ = (x); if(r_ != ncclSuccess) return ald_set_err(ALD_ERR_HIP, std::string(#x) + ": " + rccl().GetErrorString(r_)); } while(0)

} // namespace

struct ald_comm {
    ncclComm_t comm = nullptr; int world = 1, rank = 0, device = 0; hipStream_t stream = nullptr, copy_stream = nullptr;
    DevBuf d_send, d_sizes;
    // two sets of receive buffers (rank 0): while the host merges what gather k brought, gather k + 1 receives and copies into the other set
    struct Set { DevBuf d_recv; PinBuf h_recv; std::vector<int64_t> offsets; std::vector<int32_t> goffs; std::vector<hipEvent_t> landed; hipEvent_t received = nullptr; bool open = false; } set[2];
    int cur = 1;                                   // the set of the gather begun last
    // the exchange by bucket owner (ald_comm_exchange_streams) and the collection of the owners' sets (ald_comm_gather_sets): blocking, one buffer each
    DevBuf d_xrecv; std::vector<int64_t> x_seg; std::vector<int32_t> x_goffs;
};

extern "C" {

int ald_comm_unique_id(uint8_t id[128])
{
    if(!id) return ALD_ERR_INVALID;
    Rccl &R = rccl(); if(!R.ok) return ald_set_err(ALD_ERR_NO_DEVICE, R.err);
    ncclUniqueId u; NCHK(R.GetUniqueId(&u));
    static_assert(sizeof(u) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id, &u, 128);
    return ALD_OK;
}

int ald_comm_create(const uint8_t id[128], int32_t world, int32_t rank, int32_t device, ald_comm **out)
{
    if(!id || !out || world < 1 || rank < 0 || rank >= world) return ALD_ERR_INVALID;
    Rccl &R = rccl(); if(!R.ok) return ald_set_err(ALD_ERR_NO_DEVICE, R.err);
    int ndev = 0;
    if(hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ald_set_err(ALD_ERR_NO_DEVICE, "no such HIP device");
    HCHK(hipSetDevice(device));
    ald_comm *c = new ald_comm(); c->world = world; c->rank = rank; c->device = device;
    ncclUniqueId u; memcpy(&u, id, 128);
    ncclResult_t r = R.CommInitRank(&c->comm, world, u, rank);
    if(r != ncclSuccess) { delete c; return ald_set_err(ALD_ERR_HIP, std::string("ncclCommInitRank: ") + R.GetErrorString(r)); }
    if(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) { R.CommDestroy(c->comm); delete c; return ald_set_err(ALD_ERR_HIP, "stream creation failed"); }
    for(auto &st : c->set) { if(hipEventCreateWithFlags(&st.received, hipEventDisableTiming) != hipSuccess) { R.CommDestroy(c->comm); delete c; return ald_set_err(ALD_ERR_HIP, "event creation failed"); } }
    *out = c;
    return ALD_OK;
}

int ald_comm_destroy(ald_comm *c)
{
    if(!c) return ALD_OK;
    hipSetDevice(c->device);
    if(c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    if(c->copy_stream) { hipStreamSynchronize(c->copy_stream); hipStreamDestroy(c->copy_stream); }
    if(c->comm) rccl().CommDestroy(c->comm);
    c->d_send.release(); c->d_sizes.release(); c->d_xrecv.release();
    for(auto &st : c->set) { st.d_recv.release(); st.h_recv.release(); for(hipEvent_t e : st.landed) hipEventDestroy(e); if(st.received) hipEventDestroy(st.received); }
    delete c;
    return ALD_OK;
}

/* The collective in two halves.  ald_comm_gather_begin: every rank passes its stream + the global id of its first graph; the sizes are
 * exchanged (one small synchronous round), the payloads are ENQUEUED -- grouped Send / Recv to rank 0 on the communicator's stream -- and
 * on rank 0 the copy of every received stream to pinned host memory is enqueued behind them on a second stream, one copy per rank with an
 * event of its own: the call returns while the data is still on its way.  ald_comm_gather_wait(upto): blocks until the streams of ranks
 * 0..upto (-1: all; a rank other than 0: until its own send has left) have landed, then hands out the pointers.  Rank 0 can so merge
 * rank r's stream while rank r + 1's is still being copied, and -- the buffers exist twice -- begin gather k + 1 before it has merged
 * gather k: what a wait handed out stays valid until the SECOND next begin on this communicator. */
int ald_comm_gather_begin(ald_comm *c, const uint32_t *words, int64_t n_words, int32_t graph_offset)
{
    if(!c || n_words < 0 || (n_words > 0 && !words)) return ALD_ERR_INVALID;
    Rccl &R = rccl();
    HCHK(hipSetDevice(c->device));
    const int W = c->world;
    c->cur ^= 1; ald_comm::Set &S = c->set[c->cur];
    // sizes and graph offsets of every rank: one (n_words, graph_offset) pair each
    if(c->d_sizes.ensure(16 * (size_t)(W + 1))) return ald_set_err(ALD_ERR_NOMEM, "size exchange buffer");
    int64_t mine[2] = {n_words, (int64_t)graph_offset};
    HCHK(hipMemcpyAsync(c->d_sizes.p, mine, 16, hipMemcpyHostToDevice, c->stream));
    NCHK(R.AllGather(c->d_sizes.p, (char*)c->d_sizes.p + 16, 2, ncclInt64, c->comm, c->stream));
    std::vector<int64_t> all(2 * (size_t)W);
    HCHK(hipMemcpyAsync(all.data(), (char*)c->d_sizes.p + 16, 16 * (size_t)W, hipMemcpyDeviceToHost, c->stream));
    HCHK(hipStreamSynchronize(c->stream));
    S.offsets.assign((size_t)W + 1, 0); S.goffs.assign((size_t)W, 0);
    for(int r = 0; r < W; r++) { S.offsets[(size_t)r + 1] = S.offsets[(size_t)r] + all[2 * (size_t)r]; S.goffs[(size_t)r] = (int32_t)all[2 * (size_t)r + 1]; }
    // payloads: every rank sends, rank 0 receives each stream at its offset
    // a stream that already lives in HBM (ald_batch_device_transcript_stream) is sent from where it is; a host stream is staged first
    const void *src = words;
    {
        hipPointerAttribute_t at; bool on_device = false;
        if(n_words && hipPointerGetAttributes(&at, words) == hipSuccess) on_device = (at.type == hipMemoryTypeDevice);
        (void)hipGetLastError();                                   // (a plain host pointer makes the query fail: not an error here)
        if(!on_device) {
            if(c->d_send.ensure(4 * (size_t)n_words + 64)) return ald_set_err(ALD_ERR_NOMEM, "send buffer");
            if(n_words) HCHK(hipMemcpyAsync(c->d_send.p, words, 4 * (size_t)n_words, hipMemcpyHostToDevice, c->stream));
            src = c->d_send.p;
        }
    }
    const int64_t total = S.offsets[(size_t)W];
    if(c->rank == 0) {
        if(S.d_recv.ensure(4 * (size_t)total + 64) || S.h_recv.ensure(4 * (size_t)total + 64)) return ald_set_err(ALD_ERR_NOMEM, "receive buffers");
        while((int)S.landed.size() < W) { hipEvent_t e; HCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); S.landed.push_back(e); }
    }
    // the grouped section never returns between GroupStart and GroupEnd: a failed Send / Recv is remembered, the group is closed (the
    // calling thread must not stay in group mode: every later RCCL call on it would be deferred) and the stream drained -- it still
    // holds the staging copy from the caller's buffer -- before the error goes back
    {
        NCHK(R.GroupStart());
        ncclResult_t bad = ncclSuccess; const char *what = "";
        if(n_words) { const ncclResult_t r_ = R.Send(src, (size_t)n_words, ncclUint32, 0, c->comm, c->stream); if(r_ != ncclSuccess) { bad = r_; what = "ncclSend"; } }
        if(c->rank == 0) for(int r = 0; r < W && bad == ncclSuccess; r++) {
            const int64_t k = all[2 * (size_t)r]; if(!k) continue;
            const ncclResult_t r_ = R.Recv((uint32_t*)S.d_recv.p + S.offsets[(size_t)r], (size_t)k, ncclUint32, r, c->comm, c->stream);
            if(r_ != ncclSuccess) { bad = r_; what = "ncclRecv"; }
        }
        const ncclResult_t ge = R.GroupEnd();
        if(bad != ncclSuccess || ge != ncclSuccess) {
            (void)hipStreamSynchronize(c->stream);
            return ald_set_err(ALD_ERR_HIP, std::string(bad != ncclSuccess ? what : "ncclGroupEnd") + ": " + R.GetErrorString(bad != ncclSuccess ? bad : ge));
        }
    }
    HCHK(hipEventRecord(S.received, c->stream));
    if(c->rank == 0) {
        // behind the receives, on the copy stream: one D2H per rank, in rank order, an event after each -- the exchange stream is free for
        // the next gather's size round at once
        HCHK(hipStreamWaitEvent(c->copy_stream, S.received, 0));
        for(int r = 0; r < W; r++) {
            const int64_t k = all[2 * (size_t)r];
            if(k) HCHK(hipMemcpyAsync((uint32_t*)S.h_recv.p + S.offsets[(size_t)r], (const uint32_t*)S.d_recv.p + S.offsets[(size_t)r], 4 * (size_t)k, hipMemcpyDeviceToHost, c->copy_stream));
            HCHK(hipEventRecord(S.landed[(size_t)r], c->copy_stream));
        }
    }
    S.open = true;
    return ALD_OK;
}

int ald_comm_gather_wait(ald_comm *c, int32_t upto, const uint32_t **all_words, const int64_t **offsets, const int32_t **graph_offsets)
{
    if(!c) return ALD_ERR_INVALID;
    ald_comm::Set &S = c->set[c->cur];
    if(!S.open) return ald_set_err(ALD_ERR_STATE, "ald_comm_gather_wait without a gather in flight");
    HCHK(hipSetDevice(c->device));
    const int W = c->world;
    if(c->rank == 0) { const int last = (upto < 0 || upto >= W) ? W - 1 : upto; HCHK(hipEventSynchronize(S.landed[(size_t)last])); }
    else HCHK(hipEventSynchronize(S.received));
    if(all_words) *all_words = c->rank == 0 ? (const uint32_t*)S.h_recv.p : nullptr;
    if(offsets) *offsets = S.offsets.data();
    if(graph_offsets) *graph_offsets = S.goffs.data();
    return ALD_OK;
}

/* both halves in one call: rank 0 gets all streams back to back in rank order, offsets[world + 1] into them, and every rank's graph offset */
int ald_comm_gather_streams(ald_comm *c, const uint32_t *words, int64_t n_words, int32_t graph_offset,
                            const uint32_t **all_words, const int64_t **offsets, const int32_t **graph_offsets)
{
    const int rc = ald_comm_gather_begin(c, words, n_words, graph_offset);
    if(rc != ALD_OK) return rc;
    return ald_comm_gather_wait(c, -1, all_words, offsets, graph_offsets);
}

/* sizes of all ranks by one AllGather of `per` int64 each: mine[per] -> all[world * per] on the host */
static int exchange_sizes(ald_comm *c, const int64_t *mine, int per, std::vector<int64_t> &all)
{
    Rccl &R = rccl(); const int W = c->world; const size_t row = 8 * (size_t)per;
    if(c->d_sizes.ensure(row * (size_t)(W + 1))) return ald_set_err(ALD_ERR_NOMEM, "size exchange buffer");
    HCHK(hipMemcpyAsync(c->d_sizes.p, mine, row, hipMemcpyHostToDevice, c->stream));
    NCHK(R.AllGather(c->d_sizes.p, (char*)c->d_sizes.p + row, (size_t)per, ncclInt64, c->comm, c->stream));
    all.assign((size_t)W * (size_t)per, 0);
    HCHK(hipMemcpyAsync(all.data(), (char*)c->d_sizes.p + row, row * (size_t)W, hipMemcpyDeviceToHost, c->stream));
    HCHK(hipStreamSynchronize(c->stream));
    return ALD_OK;
}

/* one group of Send / Recv, closed whatever happens: n_send sends (src[i], words[i] 8- or 4-byte elements, to[i]) and n_recv receives.  A
 * failed Send / Recv is remembered, the group is closed (the calling thread must not stay in group mode) and the stream drained before
 * the error goes back -- the gather's error handling. */
struct Xfer { void *p; size_t count; int peer; };
static int grouped(ald_comm *c, ncclDataType_t type, const std::vector<Xfer> &sends, const std::vector<Xfer> &recvs)
{
    Rccl &R = rccl();
    NCHK(R.GroupStart());
    ncclResult_t bad = ncclSuccess; const char *what = "";
    for(size_t i = 0; i < sends.size() && bad == ncclSuccess; i++) { const ncclResult_t r_ = R.Send(sends[i].p, sends[i].count, type, sends[i].peer, c->comm, c->stream); if(r_ != ncclSuccess) { bad = r_; what = "ncclSend"; } }
    for(size_t i = 0; i < recvs.size() && bad == ncclSuccess; i++) { const ncclResult_t r_ = R.Recv(recvs[i].p, recvs[i].count, type, recvs[i].peer, c->comm, c->stream); if(r_ != ncclSuccess) { bad = r_; what = "ncclRecv"; } }
    const ncclResult_t ge = R.GroupEnd();
    const hipError_t he = hipStreamSynchronize(c->stream);
    if(bad != ncclSuccess || ge != ncclSuccess) return ald_set_err(ALD_ERR_HIP, std::string(bad != ncclSuccess ? what : "ncclGroupEnd") + ": " + R.GetErrorString(bad != ncclSuccess ? bad : ge));
    if(he != hipSuccess) return ald_set_err(ALD_ERR_HIP, std::string("exchange stream: ") + hipGetErrorString(he));
    return ALD_OK;
}

int ald_comm_exchange_streams(ald_comm *c, const uint32_t *words, const int64_t *offsets, int32_t graph_offset,
                              const uint32_t **dev_words, const int64_t **seg_offsets, const int32_t **graph_offsets)
{
    if(!c || !offsets || !dev_words) return ALD_ERR_INVALID;
    const int W = c->world;
    for(int r = 0; r < W; r++) if(offsets[r] < 0 || offsets[r + 1] < offsets[r]) return ald_set_err(ALD_ERR_INVALID, "ald_comm_exchange_streams: offsets must ascend");
    if(offsets[W] > offsets[0] && !words) return ALD_ERR_INVALID;
    HCHK(hipSetDevice(c->device));
    // sizes: every rank's W counts + its graph offset
    std::vector<int64_t> mine((size_t)W + 1), all;
    for(int r = 0; r < W; r++) mine[(size_t)r] = offsets[r + 1] - offsets[r];
    mine[(size_t)W] = (int64_t)graph_offset;
    { int rc = exchange_sizes(c, mine.data(), W + 1, all); if(rc != ALD_OK) return rc; }
    auto count = [&](int from, int to) { return all[(size_t)from * (size_t)(W + 1) + (size_t)to]; };
    c->x_seg.assign((size_t)W + 1, 0); c->x_goffs.assign((size_t)W, 0);
    for(int q = 0; q < W; q++) { c->x_seg[(size_t)q + 1] = c->x_seg[(size_t)q] + count(q, c->rank); c->x_goffs[(size_t)q] = (int32_t)all[(size_t)q * (size_t)(W + 1) + (size_t)W]; }
    // sub-streams that already live in HBM are sent from where they are; host memory is staged first
    const uint32_t *src = words; const int64_t n_mine = offsets[W] - offsets[0];
    if(n_mine > 0 && !tx_on_device(words)) {
        if(c->d_send.ensure(4 * (size_t)n_mine + 64)) return ald_set_err(ALD_ERR_NOMEM, "send buffer");
        HCHK(hipMemcpyAsync(c->d_send.p, words + offsets[0], 4 * (size_t)n_mine, hipMemcpyHostToDevice, c->stream));
        src = (const uint32_t*)c->d_send.p - offsets[0];
    }
    if(c->d_xrecv.ensure(4 * (size_t)c->x_seg[(size_t)W] + 64)) return ald_set_err(ALD_ERR_NOMEM, "receive buffer");
    std::vector<Xfer> sends, recvs;
    for(int q = 0; q < W; q++) {
        if(mine[(size_t)q]) sends.push_back(Xfer{(void*)(src + offsets[q]), (size_t)mine[(size_t)q], q});
        if(count(q, c->rank)) recvs.push_back(Xfer{(uint32_t*)c->d_xrecv.p + c->x_seg[(size_t)q], (size_t)count(q, c->rank), q});
    }
    { int rc = grouped(c, ncclUint32, sends, recvs); if(rc != ALD_OK) return rc; }
    *dev_words = (const uint32_t*)c->d_xrecv.p;
    if(seg_offsets) *seg_offsets = c->x_seg.data();
    if(graph_offsets) *graph_offsets = c->x_goffs.data();
    return ALD_OK;
}

int ald_comm_gather_sets(ald_comm *c, const ald_tset_flat *f, ald_tset_flat **out)
{
    if(!c || !f || !out) return ALD_ERR_INVALID;
    *out = nullptr;
    const int W = c->world;
    HCHK(hipSetDevice(c->device));
    // a bucket must live wholly on its owner: a foreign one is announced in the size exchange, and every rank leaves before anybody waits
    bool foreign = false;
    for(size_t i = 0; i < f->hash.size() && !foreign; i++) foreign = (int)(f->hash[i] % (uint64_t)W) != c->rank;
    std::vector<uint64_t> buf;
    if(!foreign) flat_pack(flat_view(*f), buf);                // (the wire form: tset_flat.h)
    int64_t mine = foreign ? -1 : (int64_t)buf.size();
    std::vector<int64_t> all;
    { int rc = exchange_sizes(c, &mine, 1, all); if(rc != ALD_OK) return rc; }
    for(int r = 0; r < W; r++) if(all[(size_t)r] < 0) return ald_set_err(ALD_ERR_INVALID, "ald_comm_gather_sets: the set of rank " + std::to_string(r) + " holds a bucket it does not own");
    std::vector<int64_t> at((size_t)W + 1, 0);
    for(int r = 0; r < W; r++) at[(size_t)r + 1] = at[(size_t)r] + all[(size_t)r];
    if(c->d_send.ensure(8 * buf.size() + 64) || (c->rank == 0 && c->d_xrecv.ensure(8 * (size_t)at[(size_t)W] + 64))) return ald_set_err(ALD_ERR_NOMEM, "set exchange buffers");
    HCHK(hipMemcpyAsync(c->d_send.p, buf.data(), 8 * buf.size(), hipMemcpyHostToDevice, c->stream));
    std::vector<Xfer> sends, recvs;
    sends.push_back(Xfer{c->d_send.p, buf.size(), 0});
    if(c->rank == 0) for(int r = 0; r < W; r++) recvs.push_back(Xfer{(uint64_t*)c->d_xrecv.p + at[(size_t)r], (size_t)all[(size_t)r], r});
    { int rc = grouped(c, ncclUint64, sends, recvs); if(rc != ALD_OK) return rc; }
    if(c->rank != 0) return ALD_OK;
    std::vector<uint64_t> got((size_t)at[(size_t)W]);
    HCHK(hipMemcpy(got.data(), c->d_xrecv.p, 8 * got.size(), hipMemcpyDeviceToHost));
    std::vector<FlatView> v((size_t)W); std::vector<HashRun> heads; int64_t N = 0, NE = 0, NS = 0;
    for(int r = 0; r < W; r++) {
        FlatView &x = v[(size_t)r];
        if(!flat_unpack(got.data() + at[(size_t)r], all[(size_t)r], x)) return ald_set_err(ALD_ERR_INVALID, "ald_comm_gather_sets: the set of rank " + std::to_string(r) + " arrived damaged");
        heads.push_back(HashRun{x.hash, x.n}); N += x.n; NE += x.ne; NS += x.ns;
    }
    // W-way merge by hash: the ranks' hashes ascend and are disjoint, so the next bucket is the smallest head, taken whole
    std::unique_ptr<ald_tset_flat> Fp(new ald_tset_flat()); ald_tset_flat *F = Fp.get();
    flat_resize(*F, N, NE, NS);
    const FlatMut Fv = flat_mut(*F); int64_t k = 0;
    for(const auto &src : merge_order(heads)) {
        const FlatView &x = v[(size_t)src.first]; const int64_t i = src.second;
        const int64_t e0 = x.exon_offset[i], e1 = x.exon_offset[i + 1], s0 = x.sample_offset[i], s1 = x.sample_offset[i + 1], eo = F->exon_offset[(size_t)k], so = F->sample_offset[(size_t)k];
        if(e0 < 0 || e1 < e0 || e1 > x.ne || s0 < 0 || s1 < s0 || s1 > x.ns || eo + (e1 - e0) > NE || so + (s1 - s0) > NS) return ald_set_err(ALD_ERR_INVALID, "ald_comm_gather_sets: inconsistent offsets in a received set");
        flat_copy_row(Fv, k++, x, i);
    }
    F->n_host_items = N;
    *out = Fp.release();
    return ALD_OK;
}

} // extern "C"
