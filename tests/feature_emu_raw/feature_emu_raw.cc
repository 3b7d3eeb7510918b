// feature_emu_raw.cc -- TEST-ONLY driver of the RAW instantiation of the batched feature routine (aletsch_amd/csrc/trst_features_dev.h) on
// one lane: graphs are staged as assembler::assemble(gx, px, sid) receives them, by the product's own HostBatch::add_graph_raw, into one
// wire buffer (as ald_batch_upload lays it out); the given paths become records of the product's layout in a pool (with a gap between
// them, as the pool of a real run has); the overlay buffers are filled with a pattern first, so that a stale weight or dead flag shows.
#ifndef ALD_EMU
#error "emulation build only"
#endif
#include "../../aletsch_amd/csrc/host_pack.h"
#include "../../aletsch_amd/csrc/trst_features_dev.h"

using namespace ald;

extern "C" {

HostBatch *femur_batch_new() { return new HostBatch(); }
void femur_batch_free(HostBatch *B) { delete B; }
int femur_batch_add_raw(HostBatch *B, const ald_graph_view *g, const ald_phase_view *ph, int32_t dist) { return B->add_graph_raw(*g, ph, dist); }
int femur_batch_add(HostBatch *B, const ald_graph_view *g) { return B->add_graph(*g); }

// paths: path_offset[n+1] (paths per graph), pv_offset[paths+1] into path_vertices; extras as ald_batch_extras (any may be null);
// lds_words: the LDS budget (0 sends every graph to the scratch).  Writes rows / complete [paths], graph_rc [n] and live_edges [n]
// (the overlay's live edge count; -2 where the wave never wrote it: staged graphs, graphs without paths).
int femur_features(HostBatch *Bp, const int64_t *path_offset, const int64_t *pv_offset, const int32_t *path_vertices, const ald_batch_extras *x, int32_t lds_words,
                   ald_trst_features *rows, int32_t *complete, int32_t *graph_rc, int32_t *live_edges)
{
    HostBatch &B = *Bp; const int n = B.n();
    HostBatch::Section sec[HostBatch::S_COUNT];
    std::vector<uint8_t> buf(B.layout(sec));
    B.pack_into(buf.data(), sec);
    const int64_t total = path_offset[n];
    // records: header + vertices, graphs in REVERSE order and 5 words of gap between records, so that nothing depends on pool order
    std::vector<unsigned long long> index((size_t)total + 1); std::vector<long long> graph_first((size_t)n, -1); std::vector<int32_t> n_paths((size_t)n, 0);
    std::vector<uint32_t> pool;
    for(int g = n - 1; g >= 0; g--) {
        n_paths[(size_t)g] = (int32_t)(path_offset[g + 1] - path_offset[g]);
        if(n_paths[(size_t)g] > 0) graph_first[(size_t)g] = path_offset[g];
        for(int64_t p = path_offset[g]; p < path_offset[g + 1]; p++) {
            pool.resize(pool.size() + 5, 0xDEADBEEFu);
            index[(size_t)p] = pool.size();
            const int k = (int)(pv_offset[p + 1] - pv_offset[p]);
            uint32_t hdr[ALD_REC_HDR] = {0}; hdr[ALD_REC_GRAPH] = (uint32_t)g; hdr[ALD_REC_PATH] = (uint32_t)(p - path_offset[g]); hdr[ALD_REC_NV] = (uint32_t)k;
            pool.insert(pool.end(), hdr, hdr + ALD_REC_HDR);
            for(int i = 0; i < k; i++) pool.push_back((uint32_t)path_vertices[pv_offset[p] + i]);
        }
    }
    std::vector<int32_t> scratch(2 * pool.size() + 64, 0x5A5A5A5A);
    std::vector<int32_t> lds(FT_LDS_WORDS, 0x5A5A5A5A);
    const size_t TE = (size_t)B.off_e[(size_t)n];
    std::vector<double> g_ew(TE + 1, -1e300); std::vector<int32_t> g_ecount(TE + 1, 0x5A5A5A5A); std::vector<uint8_t> g_dead(TE + 1, 1); std::vector<int32_t> g_live((size_t)n + 1, -2);
    FeatArgs A; memset(&A, 0, sizeof(A));
    A.in = B.make_batch_in(buf.data(), sec);
    A.pool = pool.data(); A.index = index.data(); A.graph_first = graph_first.data(); A.n_paths = n_paths.data(); A.row_begin = path_offset;
    if(x) {
        A.loss1 = x->boundary_loss1; A.loss2 = x->boundary_loss2; A.loss3 = x->boundary_loss3; A.merged_loss = x->boundary_merged_loss;
        A.leaving_count = x->unbridge_leaving_count; A.leaving_ratio = x->unbridge_leaving_ratio; A.coming_count = x->unbridge_coming_count; A.coming_ratio = x->unbridge_coming_ratio;
        A.gr_reads = x->gr_reads; A.gr_subgraph = x->gr_subgraph;
    }
    A.scratch = scratch.data(); A.lds_words = lds_words < FT_LDS_WORDS ? lds_words : FT_LDS_WORDS;
    A.rows = rows; A.complete = complete; A.graph_rc = graph_rc;
    A.g_ew = g_ew.data(); A.g_ecount = g_ecount.data(); A.g_dead = g_dead.data(); A.g_live = g_live.data();
    for(int g = 0; g < n; g++) features_graph(A, g, lds.data());
    if(live_edges) for(int g = 0; g < n; g++) live_edges[g] = g_live[(size_t)g];
    return ALD_OK;
}

} // extern "C"
