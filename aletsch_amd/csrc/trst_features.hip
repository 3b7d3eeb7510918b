// trst_features.hip -- the transcript feature block of a whole downloaded or finished batch (ald_batch_features_all): scallop::update_trst_features
// (scallop/scallop.cc:3268-3451) + unique_junc (:3472-3497), which the reference runs for every path it turns into a transcript
// (scallop::build_transcripts, :3250-3266).
//
// One wave per graph (trst_features_dev.h), FP64 throughout, on the batch's stream after a download: it reads the staged graphs (wire
// sections of d_in), the path records (d_pool) and the result index (d_index / d_gfirst) the batch already holds, plus the caller's
// extras.  The rows equal the host routine ald_batch_features (trst_features.cpp) bit for bit.  Raw graphs -- whose grouped graph exists
// only inside the decomposition kernel's raw build -- take that host routine inside the same call, on up to 16 host threads, while the
// kernel runs; their rows land in the same table.  With ALD_FEAT_RAW_ON_DEVICE (ald_batch_features_all_ex) their wave instead rebuilds
// the grouped graph as an overlay of the wire edges (trst_features_dev.h: ft_group_boundaries) and no host thread computes a row.
#include "tset_front.h"
#include "trst_features_dev.h"
#include <chrono>
#include <thread>
#include <atomic>
#include <cstdlib>

static_assert(sizeof(ald_trst_features) == 296, "ald_trst_features: the layout the Python dtype and the tests assume");

namespace {

__global__ void __launch_bounds__(64) trst_feature_waves(ald::FeatArgs A)
{
    __shared__ int32_t lds[ald::FT_LDS_WORDS];
    ald::features_graph(A, (int)blockIdx.x, lds);
}

} // namespace

extern "C" {

int ald_batch_features_all(ald_batch *b, const ald_batch_extras *x) { return ald_batch_features_all_ex(b, x, 0); }

int ald_batch_features_all_ex(ald_batch *b, const ald_batch_extras *x, uint32_t flags)
{
    if(!b) return ALD_ERR_INVALID;
    if(flags & ~ALD_FEAT_RAW_ON_DEVICE) return ald_set_err(ALD_ERR_INVALID, "ald_batch_features_all_ex: unknown flag bits");
    const bool raw_dev = (flags & ALD_FEAT_RAW_ON_DEVICE) != 0;
    if(!b->downloaded && !b->finished) return ald_set_err(ALD_ERR_STATE, "ald_batch_features_all before ald_batch_download / ald_batch_finish");
    // the host routine for raw graphs reads the downloaded records: a batch that is only finished has none
    if(!b->downloaded && !raw_dev && b->hb.has_raw) return ald_set_err(ALD_ERR_STATE, "ald_batch_features_all: a finished batch that holds raw graphs needs ALD_FEAT_RAW_ON_DEVICE (or ald_batch_download)");
    const auto T0 = std::chrono::steady_clock::now();
    FeatTable &T = b->feat;
    T.valid = false; T.device_ms = 0; T.call_ms = 0; T.device_graphs = 0; T.host_graphs = 0;
    HCHK(hipSetDevice(b->device));
    const HostBatch &hb = b->hb; const int n = hb.n();
    const int64_t rows = b->total_paths;
    const std::vector<int64_t> &path_begin = b->downloaded ? b->res.path_begin : b->path_begin;
    T.row_begin.assign(path_begin.begin(), path_begin.end());
    if(T.row_begin.empty()) T.row_begin.assign(1, 0);
    T.n_rows = rows;
    if(T.row_begin.back() != rows) return ald_set_err(ALD_ERR_STATE, "feature table: path table and path count disagree");
    const size_t RB = sizeof(ald_trst_features);
    if(T.h_rows.ensure(RB * (size_t)rows + 64, true) || T.h_complete.ensure(4 * (size_t)rows + 64, true) || T.h_rc.ensure(4 * (size_t)n + 64, true))
        return ald_set_err(ALD_ERR_NOMEM, "pinned feature table");
    int32_t *h_rc = (int32_t*)T.h_rc.p;
    std::vector<int32_t> raw;
    bool raw_paths = false;                                                      // ALD_FEAT_RAW_ON_DEVICE: some raw graph has a path, i.e. needs its overlay
    for(int g = 0; g < n; g++) if(hb.g_rawdist[(size_t)g] >= 0) { if(!raw_dev) raw.push_back(g); else if(T.row_begin[(size_t)g + 1] > T.row_begin[(size_t)g]) raw_paths = true; }
    T.host_graphs = (int64_t)raw.size(); T.device_graphs = (int64_t)n - T.host_graphs;

    // ---- the device part: every staged graph (ALD_FEAT_RAW_ON_DEVICE: every graph) with at least one path, one wave each
    const bool launch = rows > 0 && T.device_graphs > 0;
    if(launch) {
        { int rc = device_path_table(b); if(rc != ALD_OK) return rc; }          // d_pbegin: first row of every graph, from the kernel's counts
        ald::FeatArgs A; memset(&A, 0, sizeof(A));
        A.in = hb.make_batch_in((uint8_t*)b->d_in.p, b->sec);
        A.pool = (ALD_GLOBAL const uint32_t*)b->d_pool.p; A.index = (ALD_GLOBAL const unsigned long long*)b->d_index.p; A.graph_first = (ALD_GLOBAL const long long*)b->d_gfirst.p;
        A.n_paths = (ALD_GLOBAL const int32_t*)b->d_npaths.p; A.row_begin = (ALD_GLOBAL const int64_t*)b->d_pbegin.p;
        A.lds_words = ald::FT_LDS_WORDS;
        if(const char *ev = getenv("ALD_DEBUG_FEAT_LDS")) { const int k = atoi(ev); if(k >= 0 && k < ald::FT_LDS_WORDS) A.lds_words = k; }   // test knob: smaller LDS budget
        // extras to the device: per-vertex arrays [sum V], per-graph [n]
        const int64_t TV = hb.off_v[(size_t)n];
        const void *src[10] = {nullptr}; size_t bytes[10] = {0};
        if(x) {
            const void *s[10] = {x->boundary_loss1, x->boundary_loss2, x->boundary_loss3, x->boundary_merged_loss, x->unbridge_leaving_count, x->unbridge_leaving_ratio,
                                 x->unbridge_coming_count, x->unbridge_coming_ratio, x->gr_reads, x->gr_subgraph};
            const size_t w[10] = {8, 8, 8, 8, 4, 8, 4, 8, 4, 4};
            for(int k = 0; k < 10; k++) { src[k] = s[k]; bytes[k] = w[k] * (size_t)(k < 8 ? TV : n); }
        }
        const void *dev[10] = {nullptr};
        for(int k = 0; k < 10; k++) {
            if(!src[k] || !bytes[k]) continue;
            if(T.d_x[k].ensure(bytes[k])) return ald_set_err(ALD_ERR_NOMEM, "feature extras");
            HCHK(hipMemcpyAsync(T.d_x[k].p, src[k], bytes[k], hipMemcpyHostToDevice, b->stream));
            dev[k] = T.d_x[k].p;
        }
        A.loss1 = (ALD_GLOBAL const double*)dev[0]; A.loss2 = (ALD_GLOBAL const double*)dev[1]; A.loss3 = (ALD_GLOBAL const double*)dev[2]; A.merged_loss = (ALD_GLOBAL const double*)dev[3];
        A.leaving_count = (ALD_GLOBAL const int32_t*)dev[4]; A.leaving_ratio = (ALD_GLOBAL const double*)dev[5]; A.coming_count = (ALD_GLOBAL const int32_t*)dev[6]; A.coming_ratio = (ALD_GLOBAL const double*)dev[7];
        A.gr_reads = (ALD_GLOBAL const int32_t*)dev[8]; A.gr_subgraph = (ALD_GLOBAL const int32_t*)dev[9];
        // the scratch for junction lists beyond LDS: two words per word of the record pool (a path's list lies at its record's offset).
        // Only allocated when some graph may need it: a path of a graph holds at most V vertices, so (2 + 2 (V - 3)) words per path bound it.
        bool need_scratch = A.lds_words < ald::FT_LDS_WORDS;
        for(int g = 0; g < n && !need_scratch; g++) {
            const int64_t np = T.row_begin[(size_t)g + 1] - T.row_begin[(size_t)g]; const int64_t V = hb.g_nv[(size_t)g];
            if(np > 0 && 2 * np + 2 * np * (V > 3 ? V - 3 : 0) > (int64_t)A.lds_words) need_scratch = true;
        }
        if(need_scratch) {
            const uint64_t words = b->downloaded && b->res.ext_words ? b->res.ext_words : b->pool_cap_words;      // (a finished batch has no host pool: the capacity bounds it)
            if(T.d_scratch.ensure(8 * (size_t)words + 256)) return ald_set_err(ALD_ERR_NOMEM, "feature scratch");
            A.scratch = (int32_t*)T.d_scratch.p;
        }
        if(raw_paths) {                                                          // the overlay: per edge of the batch at off_e[g] + k, per graph
            const size_t TE = (size_t)hb.off_e[(size_t)n];
            if(T.d_gew.ensure(8 * TE + 64) || T.d_gecount.ensure(4 * TE + 64) || T.d_gdead.ensure(TE + 64) || T.d_glive.ensure(4 * (size_t)n + 64)) return ald_set_err(ALD_ERR_NOMEM, "feature overlay of the raw graphs");
            A.g_ew = (ALD_GLOBAL double*)T.d_gew.p; A.g_ecount = (ALD_GLOBAL int32_t*)T.d_gecount.p; A.g_dead = (ALD_GLOBAL uint8_t*)T.d_gdead.p; A.g_live = (ALD_GLOBAL int32_t*)T.d_glive.p;
        }
        if(T.d_rows.ensure(RB * (size_t)rows + 64) || T.d_complete.ensure(4 * (size_t)rows + 64) || T.d_rc.ensure(4 * (size_t)n + 64)) return ald_set_err(ALD_ERR_NOMEM, "feature table");
        A.rows = (ALD_GLOBAL ald_trst_features*)T.d_rows.p; A.complete = (ALD_GLOBAL int32_t*)T.d_complete.p; A.graph_rc = (ALD_GLOBAL int32_t*)T.d_rc.p;
        if(!T.e0) HCHK(hipEventCreate(&T.e0));
        if(!T.e1) HCHK(hipEventCreate(&T.e1));
        (void)hipGetLastError();
        HCHK(hipEventRecord(T.e0, b->stream));
        hipLaunchKernelGGL(trst_feature_waves, dim3((unsigned)n), dim3(64), 0, b->stream, A);
        if(hipGetLastError() != hipSuccess) return ald_set_err(ALD_ERR_HIP, "the feature kernel failed to launch");
        HCHK(hipEventRecord(T.e1, b->stream));
        HCHK(hipMemcpyAsync(T.h_rows.p, T.d_rows.p, RB * (size_t)rows, hipMemcpyDeviceToHost, b->stream));
        HCHK(hipMemcpyAsync(T.h_complete.p, T.d_complete.p, 4 * (size_t)rows, hipMemcpyDeviceToHost, b->stream));
        HCHK(hipMemcpyAsync(h_rc, T.d_rc.p, 4 * (size_t)n, hipMemcpyDeviceToHost, b->stream));
    }

    // ---- raw graphs: the host routine, while the kernel runs, into rows of their own; spliced in after the copies
    std::vector<ald_trst_features> raw_rows; std::vector<int32_t> raw_complete, raw_rc(raw.size(), 0); std::vector<int64_t> raw_at(raw.size() + 1, 0);
    for(size_t k = 0; k < raw.size(); k++) raw_at[k + 1] = raw_at[k] + (T.row_begin[(size_t)raw[k] + 1] - T.row_begin[(size_t)raw[k]]);
    raw_rows.resize((size_t)raw_at.back()); raw_complete.resize((size_t)raw_at.back());
    std::atomic<int> hard_err(0);
    if(!raw.empty()) {
        const double *xd[6] = {nullptr}; const int32_t *xi[4] = {nullptr};
        if(x) { xd[0] = x->boundary_loss1; xd[1] = x->boundary_loss2; xd[2] = x->boundary_loss3; xd[3] = x->boundary_merged_loss; xd[4] = x->unbridge_leaving_ratio; xd[5] = x->unbridge_coming_ratio;
                xi[0] = x->unbridge_leaving_count; xi[1] = x->unbridge_coming_count; xi[2] = x->gr_reads; xi[3] = x->gr_subgraph; }
        unsigned nthr = std::thread::hardware_concurrency(); if(nthr == 0) nthr = 1; if(nthr > 16) nthr = 16;
        if(nthr > raw.size()) nthr = (unsigned)raw.size();
        std::atomic<size_t> next(0);
        // ald_batch_features only reads the batch (the path table is built by the download), so concurrent calls on it are safe
        auto work = [&]() {
            for(size_t k; (k = next.fetch_add(1)) < raw.size(); ) {
                const int g = raw[k]; const int64_t ov = hb.off_v[(size_t)g];
                ald_graph_extras gx; memset(&gx, 0, sizeof(gx));
                auto at = [&](const double *a) { return a ? a + ov : nullptr; };
                auto ati = [&](const int32_t *a) { return a ? a + ov : nullptr; };
                gx.boundary_loss1 = at(xd[0]); gx.boundary_loss2 = at(xd[1]); gx.boundary_loss3 = at(xd[2]); gx.boundary_merged_loss = at(xd[3]);
                gx.unbridge_leaving_count = ati(xi[0]); gx.unbridge_leaving_ratio = at(xd[4]); gx.unbridge_coming_count = ati(xi[1]); gx.unbridge_coming_ratio = at(xd[5]);
                gx.gr_reads = xi[2] ? xi[2][g] : 0; gx.gr_subgraph = xi[3] ? xi[3][g] : 0;
                const int rc = ald_batch_features(b, g, &gx, raw_rows.data() + raw_at[k], raw_complete.data() + raw_at[k]);
                if(rc < 0) hard_err.store(rc);
                raw_rc[k] = rc;
            }
        };
        std::vector<std::thread> th;
        for(unsigned t = 1; t < nthr; t++) th.emplace_back(work);
        work();
        for(auto &t : th) t.join();
    }
    if(launch) {
        HCHK(hipStreamSynchronize(b->stream));
        float ms = 0; if(hipEventElapsedTime(&ms, T.e0, T.e1) == hipSuccess) T.device_ms = ms;
        if(raw_dev && !raw_paths) for(int g = 0; g < n; g++) if(hb.g_rawdist[(size_t)g] >= 0) h_rc[g] = ALD_OK;      // no overlay, no wave work: raw graphs without paths
    } else for(int g = 0; g < n; g++) h_rc[g] = ALD_OK;                    // no paths on the device side: nothing can assert
    if(hard_err.load() < 0) return ald_set_err(hard_err.load(), "ald_batch_features on a raw graph failed");
    ald_trst_features *h_rows = (ald_trst_features*)T.h_rows.p; int32_t *h_complete = (int32_t*)T.h_complete.p;
    for(size_t k = 0; k < raw.size(); k++) {
        const int g = raw[k]; const int64_t r0 = T.row_begin[(size_t)g], m = raw_at[k + 1] - raw_at[k];
        if(m > 0) { memcpy(h_rows + r0, raw_rows.data() + raw_at[k], RB * (size_t)m); memcpy(h_complete + r0, raw_complete.data() + raw_at[k], 4 * (size_t)m); }
        h_rc[g] = raw_rc[k];
    }
    T.call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    T.valid = true;
    return ALD_OK;
}

int ald_batch_features_table(const ald_batch *b, const ald_trst_features **rows, const int32_t **complete, const int32_t **graph_rc,
                             const int64_t **row_begin, int64_t *n_rows)
{
    if(!b) return ALD_ERR_INVALID;
    if((!b->downloaded && !b->finished) || !b->feat.valid) return ald_set_err(ALD_ERR_STATE, "ald_batch_features_table without ald_batch_features_all on the last download");
    const FeatTable &T = b->feat;
    if(rows) *rows = (const ald_trst_features*)T.h_rows.p;
    if(complete) *complete = (const int32_t*)T.h_complete.p;
    if(graph_rc) *graph_rc = (const int32_t*)T.h_rc.p;
    if(row_begin) *row_begin = T.row_begin.data();
    if(n_rows) *n_rows = T.n_rows;
    return ALD_OK;
}

int ald_batch_features_stats(const ald_batch *b, double *device_ms, double *call_ms, int64_t *device_graphs, int64_t *host_graphs)
{
    if(!b) return ALD_ERR_INVALID;
    if((!b->downloaded && !b->finished) || !b->feat.valid) return ald_set_err(ALD_ERR_STATE, "ald_batch_features_stats without ald_batch_features_all on the last download");
    const FeatTable &T = b->feat;
    if(device_ms) *device_ms = T.device_ms;
    if(call_ms) *call_ms = T.call_ms;
    if(device_graphs) *device_graphs = T.device_graphs;
    if(host_graphs) *host_graphs = T.host_graphs;
    return ALD_OK;
}

} // extern "C"
