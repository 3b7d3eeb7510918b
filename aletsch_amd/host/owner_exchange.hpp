// owner_exchange.hpp -- one step of a multi-process host (one process per MI355X) WITHOUT the funnel through rank 0, over the C ABI
// (include/aletsch_decomp.h).  Sits next to gpu_scallop.hpp; C++11, header only.
//
// The reference adds every graph's transcripts to the region's transcript_set under one lock (meta/assembler.cc:1127-1132).  That set is
// a map from the intron-chain hash to a bucket, and an add only ever touches one bucket (rnacore/transcript_set.cc:83-120, 149-175), so the
// set can be kept in W disjoint parts: rank r owns the buckets with hash % W == r and folds exactly their transcripts, in ascending global
// (graph, path) order -- bit for bit what the unsharded set holds for those buckets.
//
//     rank q, per batch:   ald_batch_finish(batch)                                      // or ald_batch_download
//                          aletsch::owner_exchange_fold(comm, W, batch, sid, skip, first_graph_of_q, my_set, tid_base)
//     at the end:          ald_tset_dev_snapshot(my_set, &flat); ald_comm_gather_sets(comm, flat, &all)   // rank 0: all = the region's set
//
// No rank folds more than its own buckets, about 1 / W of the transcripts.
#pragma once
#include "../../include/aletsch_decomp.h"
#include <cstdint>
#include <vector>

namespace aletsch {

// Collective; every rank calls it once per step.  Splits the finished transcripts of `batch` (downloaded or finished; NULL: this rank has
// no graphs in this step) by bucket owner on the device, exchanges the sub-streams all to all, and folds the W segments this rank
// received into `set` in rank order, i.e. in ascending global graph id.  graph_offset: global id of the batch's first graph.
// Returns ALD_OK or the first error (ald_last_error() has the text); after an error of the exchange every rank has returned one.
inline int owner_exchange_fold(ald_comm *comm, int32_t world, const ald_batch *batch, const int32_t *sid, int32_t skip_single_exon,
                               int32_t graph_offset, ald_tset_dev *set, int64_t tid_base)
{
    if(!comm || !set || world < 1 || world > 64) return ALD_ERR_INVALID;
    void *words = nullptr; const int64_t *offsets = nullptr;
    const std::vector<int64_t> none((size_t)world + 1, 0);
    int rc = ALD_OK;
    if(batch) rc = ald_batch_device_transcript_streams_by_owner(batch, sid, skip_single_exon, world, &words, &offsets);
    // a rank whose split failed still joins the collective (with nothing to send): its peers must not wait for it
    if(!batch || rc != ALD_OK) { words = nullptr; offsets = none.data(); }
    const uint32_t *recv = nullptr; const int64_t *seg = nullptr; const int32_t *goffs = nullptr;
    const int xrc = ald_comm_exchange_streams(comm, (const uint32_t*)words, offsets, graph_offset, &recv, &seg, &goffs);
    if(rc != ALD_OK) return rc;
    if(xrc != ALD_OK) return xrc;
    for(int32_t q = 0; q < world; q++) {
        const int64_t n = seg[q + 1] - seg[q];
        if(n == 0) continue;
        rc = ald_tset_dev_add_stream(set, recv + seg[q], n, nullptr, nullptr, goffs[q], tid_base, 0 /* left out by the split already */);
        if(rc != ALD_OK) return rc;
    }
    return ALD_OK;
}

} // namespace aletsch
