// input_expand.h -- compact input: the sections of the device input buffer that ald_batch_upload did NOT copy (HostBatch::layout marked
// them `derived`), filled on the device from the sections that did travel.  Kernels + their host launcher in a header: the library
// includes it through input_expand.hip, the byte-comparison program of the GPU tier (tests/compact_input_gpu_main.hip) directly.
//
// One wavefront per graph (blockDim 64), in this order:
//   sample lists   edge_sample_offset[k] = k, sample_id[k] = the graph's one sample id, sample_abd[k] = edge_weight[k] (the same bits)
//   edge_abd       the in-order sum of the edge's sample_abd, starting from +0.0 as the host does (no reassociation; a single -0.0 gives +0.0)
//   edge_count     the number of samples of the edge
//   in-CSR         counting sort of edge ids by target, ids ascending inside every in-list
// and two memsets (edge_strand = 0, vertex_type = -1).  A step reads only columns that travelled (edge_abd / edge_count of a batch whose
// sample lists are derived too are made from edge_weight, not from the lists the same kernel writes) plus the per-graph sample ids.
//
// The in-CSR uses ONE array of V + 1 counters c[]: targets are counted into c[t + 2], an inclusive scan makes c[t + 1] the first slot of
// target t, the placement advances c[t + 1] past the slots it hands out, which leaves c[] = in_offset.  The placement walks the edges 64
// at a time in id order; inside a group a lane's slot is c[t + 1] + (lower lanes with the same target), found with 63 rotations of the
// target through the wave -- no atomic decides an order, so the result is the host's counting sort whatever the scheduling.
// ONE form for every graph (any size: add takes graphs far beyond the largest class): c[] IS the graph's in_offset slots in global memory.
// No LDS, no scratch buffer, and at most ALD_EXPAND_VGPRS registers per lane -- on purpose.  A pipelined caller uploads batch k + 1 while
// the persistent class kernels of batch k hold the CUs: the class-1 kernel (the bench shape) keeps 20 workgroups of 8 184 B on a CU --
// 163 520 of its 163 840 B of LDS -- and 5 x 96 of a SIMD's 512 VGPRs.  An expand wave that asks for 4 KB of LDS, as the first form of
// this kernel did, gets on a CU only when class workgroups retire (upload 33 ms instead of 24 in bench.py's loop); one that asks for no
// LDS and 32 VGPRs fits into what that kernel leaves free.
#pragma once
#include <hip/hip_runtime.h>
#include "host_pack.h"

namespace ald {

enum { ALD_EXPAND_VGPRS = 32 };
#if defined(__HIPCC__)
// c[0 .. V]: the graph's in_offset slots.  tg: the graph's E targets, ie: its E in_edge slots.
__device__ __forceinline__ void expand_in_csr(ALD_GLOBAL int32_t *c, ALD_GLOBAL const int32_t *tg, ALD_GLOBAL int32_t *ie, int V, int E, int lane)
{
    for(int i = lane; i <= V; i += 64) c[i] = 0;
    wsync_mem();
    for(int k = lane; k < E; k += 64) { const int t = tg[k]; if(t >= 0 && t + 2 <= V) __hip_atomic_fetch_add(&c[t + 2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }      // (the sink's count is never needed)
    wsync_mem();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // the counts were made by atomics in L2, the scan reads them with plain loads
    int carry = 0;                                   // inclusive scan of c[1 .. V], 64 entries at a time
    for(int base = 1; base <= V; base += 64) {
        const int i = base + lane; int x = i <= V ? c[i] : 0;
        for(int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if(lane >= d) x += y; }
        x += carry;
        if(i <= V) c[i] = x;
        carry = __shfl(x, 63, 64);
    }
    wsync_mem();
    for(int base = 0; base < E; base += 64) {
        const int k = base + lane; const bool on = k < E;
        const int t = on ? tg[k] : -1 - lane;        // (an idle lane matches nobody)
        int below = 0, above = 0;
        for(int d = 1; d < 64; d++) { const int src = (lane + d) & 63; const int y = __shfl(t, src, 64); if(y == t) { if(src < lane) below++; else above++; } }
        const bool ok = on && t >= 0 && t < V;
        const int pos = ok ? c[t + 1] + below : 0;
        wsync_mem();                                 // every lane of the group has its first slot before the last lane of a target moves it
        if(ok && pos < E) ie[pos] = k;
        if(ok && above == 0) c[t + 1] = pos + 1;
        wsync_mem();
    }
}

// (gsid_: a plain pointer in the signature -- ALD_GLOBAL is an address space in the device pass only, and a kernel's mangled name must be
// the same in both passes for the host to find it)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(ALD_EXPAND_VGPRS))) expand_graphs(BatchIn in, const int32_t *gsid_, unsigned derive)
{
    ALD_GLOBAL const int32_t *gsid = (ALD_GLOBAL const int32_t*)gsid_;
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    if(g >= in.n_graphs) return;
    const int V = in.g_nv[g], E = in.g_ne[g];
    const int64_t oe = in.off_e[g], os = in.off_s[g], ovo = in.off_v[g] + g, oeo = oe + g;
    ALD_GLOBAL const double *ew = in.edge_weight + oe;
    if(derive & ALD_DERIVE_SAMPLES) {
        ALD_GLOBAL int32_t *so = (ALD_GLOBAL int32_t*)in.edge_sample_offset + oeo, *sid = (ALD_GLOBAL int32_t*)in.sample_id + os; ALD_GLOBAL double *sabd = (ALD_GLOBAL double*)in.sample_abd + os;
        const int32_t id = gsid[g];
        for(int k = lane; k <= E; k += 64) { so[k] = k; if(k < E) { sid[k] = id; sabd[k] = ew[k]; } }
    }
    if(derive & ALD_DERIVE_EABD) {
        ALD_GLOBAL double *eabd = (ALD_GLOBAL double*)in.edge_abd + oe;
        if(derive & ALD_DERIVE_SAMPLES) for(int k = lane; k < E; k += 64) { double sum = 0; sum += ew[k]; eabd[k] = sum; }
        else {
            ALD_GLOBAL const int32_t *so = in.edge_sample_offset + oeo; ALD_GLOBAL const double *sabd = in.sample_abd + os;
            for(int k = lane; k < E; k += 64) { double sum = 0; for(int j = so[k]; j < so[k + 1]; j++) sum += sabd[j]; eabd[k] = sum; }
        }
    }
    if(derive & ALD_DERIVE_ECOUNT) {
        ALD_GLOBAL int32_t *ec = (ALD_GLOBAL int32_t*)in.edge_count + oe;
        if(derive & ALD_DERIVE_SAMPLES) for(int k = lane; k < E; k += 64) ec[k] = 1;
        else { ALD_GLOBAL const int32_t *so = in.edge_sample_offset + oeo; for(int k = lane; k < E; k += 64) ec[k] = so[k + 1] - so[k]; }
    }
    if(derive & ALD_DERIVE_INCSR) {
        ALD_GLOBAL int32_t *io = (ALD_GLOBAL int32_t*)in.in_offset + ovo, *ie = (ALD_GLOBAL int32_t*)in.in_edge + oe;
        expand_in_csr(io, in.edge_target + oe, ie, V, E, lane);
    }
}

// Enqueues the expansion on `st`, behind the copies of the sections that travel.  in: BatchIn of DEVICE pointers (make_batch_in);
// d_gsid: one sample id per graph on the device (read only with ALD_DERIVE_SAMPLES); total_v / total_e: vertices / edges of the batch.
inline hipError_t expand_input(const BatchIn &in, const int32_t *d_gsid, int64_t total_v, int64_t total_e, unsigned derive, hipStream_t st)
{
    if(!derive || in.n_graphs <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if((derive & ALD_DERIVE_ESTRAND) && total_e > 0) e = hipMemsetAsync((void*)in.edge_strand, 0, (size_t)total_e, st);
    if(e == hipSuccess && (derive & ALD_DERIVE_VTYPE) && total_v > 0) e = hipMemsetAsync((void*)in.vertex_type, 0xFF, 4 * (size_t)total_v, st);      // -1
    if(e != hipSuccess) return e;
    if(derive & (ALD_DERIVE_INCSR | ALD_DERIVE_SAMPLES | ALD_DERIVE_EABD | ALD_DERIVE_ECOUNT)) {
        hipLaunchKernelGGL(expand_graphs, dim3((unsigned)in.n_graphs), dim3(64), 0, st, in, d_gsid, derive);
        e = hipGetLastError();
    }
    return e;
}
#endif

} // namespace ald
