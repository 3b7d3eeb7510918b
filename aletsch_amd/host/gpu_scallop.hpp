// gpu_scallop.hpp -- C++ host adapter over the C ABI (include/aletsch_decomp.h) with the reference's call surface.
//
// The reference decomposes one graph with (meta/assembler.cc:1110-1121, scallop/scallop.h:31-51):
//
//     scallop sx(gx, hx, pa, false);     // ctor: splice_graph&, hyper_set&, const parameters&, bool random_ordering
//     sx.assemble();                     // int, always 0
//     for(transcript &t : sx.trsts) ...  // public: vector<path> paths; vector<transcript> trsts;
//
// aletsch::gpu_scallop keeps exactly that two-call shape (single graph = a batch of one), and
// aletsch::gpu_scallop_batch lifts it to many graphs per launch, which is where the MI355X pays off: the dispatch
// loops (meta/incubator.cc:609-637, meta/assembler.cc:296-347,370) enqueue (graph, phasing set) pairs, flush() runs
// them in one batch, and result(i) hands back what `sx.paths` would have held for graph i.
//
// The adapter is a template over the reference's own types so that it compiles INSIDE the reference tree with its
// headers (splice_graph.h, hyper_set.h, parameters.h, path.h) and needs none of them here.  Duck-typed members used:
//   SpliceGraph: num_vertices(), edges() -> pair<edge_iterator,edge_iterator> over edge_descriptor (with ->source(),
//                ->target()), get_edge_weight(e), get_edge_info(e) {.strand,.count,.abd,.samples,.spAbd},
//                get_vertex_weight(v), get_vertex_info(v) {.lpos,.rpos,.type}, .strand
//   HyperSet:    .nodes  (map<vector<int>, int>: vertex lists -> count, after the ctor + filter_nodes)
//   Parameters:  .max_decompose_error_ratio[8], .min_guaranteed_edge_weight, .min_transcript_coverage, .max_num_exons
//   Path:        .v, .junc, .length, .abd, .weight, .conf, .reads, .strand, .count      (rnacore/path.h)
//
// Canonical edge order: the reference's order is raw-pointer order, which is what gr.edges() iterates in and what
// scallop's ctor turns into edge indices (scallop.cc:24, graph_base.cc:139-153).  The adapter lays the edges out as CSR by
// (source, target, position in gr.edges()) -- the order each vertex's out-edge set iterates in -- and hands the position in
// gr.edges() over as ald_graph_view.edge_creation_rank, so that the kernel's edge ids ARE the reference's e2i values.
// The consumed-input contract is relaxed: gx / hx are left untouched (the reference empties them; its callers never read
// them again: assembler.cc:346-355).
#pragma once
#include "../../include/aletsch_decomp.h"
#include <vector>
#include <map>
#include <algorithm>
#include <stdexcept>
#include <string>
#include <cstdint>
#include <type_traits>

namespace aletsch {

struct staged_graph {                       // owning arrays behind one ald_graph_view
    std::vector<int32_t> vertex_offset, edge_target, edge_sample_offset, sample_id, vertex_lpos, vertex_rpos, vertex_type, phasing_offset, phasing_vertex, phasing_count, edge_count, edge_rank;
    std::vector<double> edge_weight, edge_abd, sample_abd, vertex_weight; std::vector<uint8_t> edge_strand; char strand = '.';
    ald_graph_view view() const {
        ald_graph_view g{};
        g.num_vertices = (int32_t)vertex_weight.size(); g.num_edges = (int32_t)edge_target.size();
        g.vertex_offset = vertex_offset.data(); g.edge_target = edge_target.data(); g.edge_weight = edge_weight.data(); g.edge_strand = edge_strand.data(); g.edge_abd = edge_abd.data();
        g.edge_sample_offset = edge_sample_offset.data(); g.sample_id = sample_id.data(); g.sample_abd = sample_abd.data();
        g.vertex_weight = vertex_weight.data(); g.vertex_lpos = vertex_lpos.data(); g.vertex_rpos = vertex_rpos.data(); g.vertex_type = vertex_type.data();
        g.num_phasing = (int32_t)phasing_count.size(); g.phasing_offset = phasing_offset.data(); g.phasing_vertex = phasing_vertex.data(); g.phasing_count = phasing_count.data();
        g.strand = strand; g.edge_count = edge_count.data(); g.edge_creation_rank = edge_rank.empty() ? nullptr : edge_rank.data();
        return g;
    }
};

template<class SpliceGraph, class HyperSet>
staged_graph stage_graph(SpliceGraph &gr, const HyperSet &hs)
{
    staged_graph s;
    const int V = (int)gr.num_vertices();
    typedef typename std::decay<decltype(*gr.edges().first)>::type edge_t;     // edge_descriptor
    struct E { int src, dst, ord; edge_t e; };
    std::vector<E> es; es.reserve(256);
    { auto pe = gr.edges(); int k = 0; for(auto it = pe.first; it != pe.second; ++it, ++k) es.push_back(E{(*it)->source(), (*it)->target(), k, *it}); }
    std::stable_sort(es.begin(), es.end(), [](const E &a, const E &b) { return a.src != b.src ? a.src < b.src : (a.dst != b.dst ? a.dst < b.dst : a.ord < b.ord); });
    s.vertex_offset.assign(V + 1, 0);
    for(const E &x : es) s.vertex_offset[x.src + 1]++;
    for(int i = 0; i < V; i++) s.vertex_offset[i + 1] += s.vertex_offset[i];
    { const size_t ne = es.size();                              // one allocation per array instead of a doubling series
      s.edge_target.reserve(ne); s.edge_weight.reserve(ne); s.edge_strand.reserve(ne); s.edge_abd.reserve(ne); s.edge_count.reserve(ne); s.edge_rank.reserve(ne);
      s.edge_sample_offset.reserve(ne + 1); s.sample_id.reserve(ne); s.sample_abd.reserve(ne);
      s.vertex_weight.reserve((size_t)V); s.vertex_lpos.reserve((size_t)V); s.vertex_rpos.reserve((size_t)V); s.vertex_type.reserve((size_t)V); }
    s.edge_sample_offset.push_back(0);
    for(const E &x : es) {
        const auto &ei = gr.get_edge_info(x.e);
        s.edge_target.push_back(x.dst); s.edge_weight.push_back(gr.get_edge_weight(x.e)); s.edge_strand.push_back((uint8_t)ei.strand); s.edge_abd.push_back(ei.abd);
        // edge_info.count travels as its own field: it starts as the number of supporting samples (meta/assembler.cc:202-231) but
        // group_start_boundaries ADDS counts along a grouped boundary (graph_reviser.cc:965-975) without touching the sample sets
        s.edge_count.push_back((int32_t)ei.count);
        s.edge_rank.push_back((int32_t)x.ord);          // scallop's edge index of this edge: get_edge_indices numbers gr.edges() in iteration order (graph_base.cc:139-153)
        for(int sp : ei.samples) { s.sample_id.push_back(sp); auto f = ei.spAbd.find(sp); s.sample_abd.push_back(f == ei.spAbd.end() ? 0.0 : f->second); }
        s.edge_sample_offset.push_back((int32_t)s.sample_id.size());
    }
    for(int i = 0; i < V; i++) { const auto &vi = gr.get_vertex_info(i); s.vertex_weight.push_back(gr.get_vertex_weight(i)); s.vertex_lpos.push_back(vi.lpos); s.vertex_rpos.push_back(vi.rpos); s.vertex_type.push_back(vi.type); }
    s.phasing_offset.push_back(0);
    for(const auto &kv : hs.nodes) { for(int x : kv.first) s.phasing_vertex.push_back(x); s.phasing_offset.push_back((int32_t)s.phasing_vertex.size()); s.phasing_count.push_back(kv.second); }
    s.strand = gr.strand;
    return s;
}

class gpu_error : public std::runtime_error {
public:
    int code;
    gpu_error(int c, const char *what) : std::runtime_error(std::string("aletsch_decomp: ") + what + " (" + std::to_string(c) + "): " + ald_last_error()), code(c) {}
};

// assembler::assemble(gx, px, sid) up to `scallop sx(gx, hx, pa)` (meta/assembler.cc:1075-1086): extend_strands, boundary grouping,
// phase projection, hyper_set(gx, px), filter_nodes -- done by the library (ald_pre_assemble) on the staged arrays; gx and px are left
// untouched.  PhaseSet: .pmap (map<vector<int32_t>, int>, rnacore/phase_set.h:24).  `status` receives 0, or the positive status word
// where the reference would have asserted in those steps (the returned graph is empty then).
template<class SpliceGraph, class PhaseSet>
staged_graph stage_raw(SpliceGraph &gx, const PhaseSet &px, int max_group_boundary_distance, int &status)
{
    struct no_hyper_set { std::map<std::vector<int>, int> nodes; } none;
    staged_graph in = stage_graph(gx, none);
    std::vector<int32_t> off(1, 0), coord, cnt;
    for(const auto &kv : px.pmap) { coord.insert(coord.end(), kv.first.begin(), kv.first.end()); off.push_back((int32_t)coord.size()); cnt.push_back((int32_t)kv.second); }
    static const int32_t zero = 0;
    ald_phase_view pv; pv.num_phases = (int32_t)cnt.size(); pv.phase_offset = off.data(); pv.phase_coord = coord.empty() ? &zero : coord.data(); pv.phase_count = cnt.empty() ? &zero : cnt.data();
    ald_graph_view gv = in.view();
    ald_staged *S = nullptr;
    status = ald_pre_assemble(&gv, &pv, max_group_boundary_distance, &S);
    if(status < 0) throw gpu_error(status, "ald_pre_assemble");
    staged_graph out;
    if(status > 0) return out;
    ald_graph_view v; ald_staged_view(S, &v);
    const int V = v.num_vertices, E = v.num_edges, P = v.num_phasing;
    const int NS = E > 0 ? v.edge_sample_offset[E] : 0, NPV = P > 0 ? v.phasing_offset[P] : 0;
    out.vertex_offset.assign(v.vertex_offset, v.vertex_offset + V + 1); out.edge_target.assign(v.edge_target, v.edge_target + E); out.edge_weight.assign(v.edge_weight, v.edge_weight + E);
    out.edge_strand.assign(v.edge_strand, v.edge_strand + E); out.edge_abd.assign(v.edge_abd, v.edge_abd + E); out.edge_sample_offset.assign(v.edge_sample_offset, v.edge_sample_offset + E + 1);
    out.sample_id.assign(v.sample_id, v.sample_id + NS); out.sample_abd.assign(v.sample_abd, v.sample_abd + NS);
    out.vertex_weight.assign(v.vertex_weight, v.vertex_weight + V); out.vertex_lpos.assign(v.vertex_lpos, v.vertex_lpos + V); out.vertex_rpos.assign(v.vertex_rpos, v.vertex_rpos + V);
    out.vertex_type.assign(v.vertex_type, v.vertex_type + V); out.phasing_offset.assign(v.phasing_offset, v.phasing_offset + P + 1); out.phasing_vertex.assign(v.phasing_vertex, v.phasing_vertex + NPV);
    out.phasing_count.assign(v.phasing_count, v.phasing_count + P); out.edge_count.assign(v.edge_count, v.edge_count + E);
    if(v.edge_creation_rank) out.edge_rank.assign(v.edge_creation_rank, v.edge_creation_rank + E);
    out.strand = v.strand;
    ald_staged_free(S);
    return out;
}

// compact input (ALD_PARAM_COMPACT_INPUT): a configuration that has a `compact_input` member switches it on with it; the reference's own
// parameters class has none and keeps the full upload
template<class Parameters> auto compact_input_of(const Parameters &cfg, int) -> decltype((bool)cfg.compact_input) { return (bool)cfg.compact_input; }
template<class Parameters> bool compact_input_of(const Parameters &, long) { return false; }
template<class Parameters>
ald_params stage_params(const Parameters &cfg)
{
    ald_params p;
    for(int i = 0; i < 8; i++) p.max_decompose_error_ratio[i] = cfg.max_decompose_error_ratio[i];
    p.min_guaranteed_edge_weight = cfg.min_guaranteed_edge_weight; p.min_transcript_coverage = cfg.min_transcript_coverage;
    p.max_num_exons = cfg.max_num_exons; p.reserved = compact_input_of(cfg, 0) ? ALD_PARAM_COMPACT_INPUT : 0;
    return p;
}

// what scallop::collect_path fills (scallop.cc:2797-2822), including the junction list derived from the ORIGINAL coordinates
template<class Path>
Path make_path(const ald_path_view &pv, const std::vector<int32_t> &lpos, const std::vector<int32_t> &rpos)
{
    Path p;
    p.v.assign(pv.vertices, pv.vertices + pv.num_vertices);
    p.length = pv.length; p.weight = pv.weight; p.abd = pv.abd; p.conf = pv.conf; p.reads = pv.reads; p.count = pv.count; p.strand = pv.strand;
    p.junc.clear();
    for(int i = 2; i + 1 < pv.num_vertices; i++) if(lpos[p.v[i]] != rpos[p.v[i - 1]]) p.junc.push_back(std::make_pair(p.v[i - 1], p.v[i]));
    return p;
}

// many graphs per launch
template<class SpliceGraph, class HyperSet, class Parameters, class Path>
class gpu_scallop_batch {
public:
    explicit gpu_scallop_batch(const Parameters &cfg, int device = 0) {
        ald_params p = stage_params(cfg);
        int rc = ald_batch_create(&p, device, &b_);
        if(rc != ALD_OK) throw gpu_error(rc, "ald_batch_create");
    }
    ~gpu_scallop_batch() { if(b_) ald_batch_destroy(b_); }
    gpu_scallop_batch(const gpu_scallop_batch &) = delete;
    gpu_scallop_batch &operator=(const gpu_scallop_batch &) = delete;

    // returns the index under which the graph's result will be available after flush()
    int enqueue(SpliceGraph &gr, const HyperSet &hs) {
        staged_graph s = stage_graph(gr, hs);
        ald_graph_view g = s.view();
        int rc = ald_batch_add_graph(b_, &g);
        if(rc != ALD_OK) throw gpu_error(rc, "ald_batch_add_graph");
        lpos_.push_back(std::move(s.vertex_lpos)); rpos_.push_back(std::move(s.vertex_rpos));
        return (int)lpos_.size() - 1;
    }
    // the same for a graph as assembler::assemble(gx, px, sid) receives it: its pre-steps (meta/assembler.cc:1075-1086) run on the device,
    // in the wave that loads the graph.  Returns the ticket; where the reference would have asserted in them status(ticket) says so.
    template<class PhaseSet>
    int enqueue_raw(SpliceGraph &gx, const PhaseSet &px, int max_group_boundary_distance = 10000) {
        struct no_hyper_set { std::map<std::vector<int>, int> nodes; } none;
        staged_graph s = stage_graph(gx, none);                      // the graph as it is; the pre-steps run on the device (ald_batch_add_graph_raw)
        std::vector<int32_t> off(1, 0), coord, cnt;
        for(const auto &kv : px.pmap) { coord.insert(coord.end(), kv.first.begin(), kv.first.end()); off.push_back((int32_t)coord.size()); cnt.push_back((int32_t)kv.second); }
        static const int32_t zero = 0;
        ald_phase_view pv; pv.num_phases = (int32_t)cnt.size(); pv.phase_offset = off.data(); pv.phase_coord = coord.empty() ? &zero : coord.data(); pv.phase_count = cnt.empty() ? &zero : cnt.data();
        ald_graph_view g = s.view();
        int rc = ald_batch_add_graph_raw(b_, &g, &pv, max_group_boundary_distance);
        if(rc != ALD_OK) throw gpu_error(rc, "ald_batch_add_graph_raw");
        lpos_.push_back(std::move(s.vertex_lpos)); rpos_.push_back(std::move(s.vertex_rpos));
        return (int)lpos_.size() - 1;
    }
    void flush() {
        int rc; status_.clear();
        if((rc = ald_batch_upload(b_)) != ALD_OK) throw gpu_error(rc, "ald_batch_upload");
        if((rc = ald_batch_run(b_)) != ALD_OK) throw gpu_error(rc, "ald_batch_run");
        if((rc = ald_batch_download(b_)) != ALD_OK) throw gpu_error(rc, "ald_batch_download");
    }
    // upload, run and END the run on the device (ald_batch_finish): the records stay in HBM.  For a caller whose consumers read them there --
    // ald_tset_dev_add_batch(set, handle(), ...), ald_batch_device_transcript_stream, features() -- and who does not read paths(); status(i)
    // works after either flush, paths(i) needs flush() (or ald_batch_download(handle()) afterwards, which then only fetches the records).
    void flush_on_device() {
        int rc;
        if((rc = ald_batch_upload(b_)) != ALD_OK) throw gpu_error(rc, "ald_batch_upload");
        if((rc = ald_batch_run(b_)) != ALD_OK) throw gpu_error(rc, "ald_batch_run");
        if((rc = ald_batch_finish(b_)) != ALD_OK) throw gpu_error(rc, "ald_batch_finish");
        status_.assign(lpos_.size(), -1);
        if(!status_.empty() && (rc = ald_batch_export_status(b_, status_.data(), nullptr, nullptr)) != ALD_OK) throw gpu_error(rc, "ald_batch_export_status");
    }
    // per-graph status word (ALD_ST_*): the reference would have aborted on an assert where this is >= ALD_ST_INVARIANT
    int status(int i) const {
        ald_result_view r;
        if(ald_batch_get_result(b_, i, &r) == ALD_OK) return r.status;
        return i >= 0 && i < (int)status_.size() ? (int)status_[(size_t)i] : -1;      // after flush_on_device()
    }
    std::vector<Path> paths(int i) const {
        ald_result_view r;
        int rc = ald_batch_get_result(b_, i, &r);
        if(rc != ALD_OK) throw gpu_error(rc, "ald_batch_get_result");
        std::vector<Path> out;
        for(int k = 0; k < r.num_paths; k++) { ald_path_view pv; ald_batch_get_path(b_, i, k, &pv); out.push_back(make_path<Path>(pv, lpos_[i], rpos_[i])); }
        return out;
    }
    void clear() { ald_batch_clear(b_); lpos_.clear(); rpos_.clear(); extras_.clear(); status_.clear(); }
    ald_batch *handle() const { return b_; }        // for the calls that take the batch itself (ald_tset_add_batch, ald_batch_export_transcripts, ...)

    // ---- the transcript feature block (scallop::update_trst_features, scallop.cc:3268-3451), opt-in.  Member templates: instantiated only
    // where they are used, so graph types without the feature members (vertex_info's boundary / unbridged fields, splice_graph::reads /
    // subgraph) still work with everything above.
    // enqueue() / enqueue_raw() that also record what the features read beyond the decomposition's inputs, from the graph's own objects
    // (rnacore/vertex_info.h:34-41, splice_graph.h:36-37).  A graph enqueued without them reads zeros there.
    template<class G>
    int enqueue_with_extras(G &gr, const HyperSet &hs) { const int t = enqueue(gr, hs); record_extras(t, gr); return t; }
    template<class G, class PhaseSet>
    int enqueue_raw_with_extras(G &gx, const PhaseSet &px, int max_group_boundary_distance = 10000) { const int t = enqueue_raw(gx, px, max_group_boundary_distance); record_extras(t, gx); return t; }
    // After flush(): the features of every path of ticket i, in path order, in a caller type F with the field names of the reference's
    // transcript::TrstFeatures (gtf/transcript.h:60-104) -- what build_transcripts puts into trst.features before ts.add.  The whole batch
    // is computed by the first call after a flush (ald_batch_features_all_ex: one device pass; raw graphs by the host routine, or, after
    // features_raw_on_device(true), by the same device pass).  `status`
    // receives what the reference's asserts would have said (ALD_OK, or ALD_ST_INVARIANT + ALD_INV_OTHER); `complete` (optional): 0 for
    // a path without a junction, whose fields past the first seven the reference never sets.
    // raw tickets (enqueue_raw) in the device pass as well (ALD_FEAT_RAW_ON_DEVICE): the kernel folds their boundaries itself instead of the
    // host re-running the pre-steps per graph.  Same values; takes effect at the next computation of the table.  Default: false.
    void features_raw_on_device(bool on) { feat_raw_on_device_ = on; }
    template<class F>
    std::vector<F> features(int i, int *status = nullptr, std::vector<int> *complete = nullptr) {
        const ald_trst_features *rows = nullptr; const int32_t *comp = nullptr, *rc = nullptr; const int64_t *rb = nullptr; int64_t nr = 0;
        if(ald_batch_features_table(b_, &rows, &comp, &rc, &rb, &nr) != ALD_OK) {
            compute_features();
            int r = ald_batch_features_table(b_, &rows, &comp, &rc, &rb, &nr);
            if(r != ALD_OK) throw gpu_error(r, "ald_batch_features_table");
        }
        if(i < 0 || i >= (int)lpos_.size()) throw gpu_error(ALD_ERR_INVALID, "features: no such ticket");
        std::vector<F> out;
        if(status) *status = rc[i];
        if(complete) complete->clear();
        for(int64_t k = rb[i]; k < rb[i + 1]; k++) {
            const ald_trst_features &x = rows[k]; F f;
            f.gr_vertices = x.gr_vertices; f.gr_edges = x.gr_edges; f.gr_reads = x.gr_reads; f.gr_subgraph = x.gr_subgraph; f.num_vertices = x.num_vertices; f.num_edges = x.num_edges;
            f.junc_ratio = x.junc_ratio; f.max_mid_exon_len = x.max_mid_exon_len;
            f.start_loss1 = x.start_loss1; f.start_loss2 = x.start_loss2; f.start_loss3 = x.start_loss3; f.end_loss1 = x.end_loss1; f.end_loss2 = x.end_loss2; f.end_loss3 = x.end_loss3;
            f.start_merged_loss = x.start_merged_loss; f.end_merged_loss = x.end_merged_loss;
            f.introns = x.introns; f.start_introns = x.start_introns; f.end_introns = x.end_introns; f.intron_ratio = x.intron_ratio; f.start_intron_ratio = x.start_intron_ratio; f.end_intron_ratio = x.end_intron_ratio;
            f.uni_junc = x.uni_junc;
            f.seq_min_wt = x.seq_min_wt; f.seq_min_cnt = x.seq_min_cnt; f.seq_min_abd = x.seq_min_abd; f.seq_min_ratio = x.seq_min_ratio;
            f.seq_max_wt = x.seq_max_wt; f.seq_max_cnt = x.seq_max_cnt; f.seq_max_abd = x.seq_max_abd; f.seq_max_ratio = x.seq_max_ratio;
            f.unbridge_start_coming_count = x.unbridge_start_coming_count; f.unbridge_start_coming_ratio = x.unbridge_start_coming_ratio;
            f.unbridge_end_leaving_count = x.unbridge_end_leaving_count; f.unbridge_end_leaving_ratio = x.unbridge_end_leaving_ratio;
            f.start_cnt = x.start_cnt; f.start_weight = x.start_weight; f.start_abd = x.start_abd; f.end_cnt = x.end_cnt; f.end_weight = x.end_weight; f.end_abd = x.end_abd;
            out.push_back(f);
            if(complete) complete->push_back(comp[k]);
        }
        return out;
    }
private:
    struct graph_extras { std::vector<double> loss1, loss2, loss3, merged, leaving_ratio, coming_ratio; std::vector<int32_t> leaving_count, coming_count; int32_t reads = 0, subgraph = 0; };
    template<class G>
    void record_extras(int t, G &gr) {
        if((int)extras_.size() <= t) extras_.resize((size_t)t + 1);
        graph_extras &x = extras_[(size_t)t];
        const int V = (int)gr.num_vertices();
        for(int v = 0; v < V; v++) {
            const auto &vi = gr.get_vertex_info(v);
            x.loss1.push_back(vi.boundary_loss1); x.loss2.push_back(vi.boundary_loss2); x.loss3.push_back(vi.boundary_loss3); x.merged.push_back(vi.boundary_merged_loss);
            x.leaving_count.push_back((int32_t)vi.unbridge_leaving_count); x.leaving_ratio.push_back(vi.unbridge_leaving_ratio);
            x.coming_count.push_back((int32_t)vi.unbridge_coming_count); x.coming_ratio.push_back(vi.unbridge_coming_ratio);
        }
        x.reads = (int32_t)gr.reads; x.subgraph = (int32_t)gr.subgraph;
    }
    // the batch's extras, flat (graphs back to back in ticket order; zeros for a ticket enqueued without them), then the device pass
    void compute_features() {
        const size_t n = lpos_.size(); size_t TV = 0;
        for(size_t t = 0; t < n; t++) TV += lpos_[t].size();
        std::vector<double> l1(TV, 0.0), l2(TV, 0.0), l3(TV, 0.0), lm(TV, 0.0), lr(TV, 0.0), cr(TV, 0.0); std::vector<int32_t> lc(TV, 0), cc(TV, 0), rd(n, 0), sg(n, 0);
        size_t at = 0;
        for(size_t t = 0; t < n; t++) {
            const size_t V = lpos_[t].size();
            if(t < extras_.size() && extras_[t].loss1.size() == V) {
                const graph_extras &x = extras_[t];
                std::copy(x.loss1.begin(), x.loss1.end(), l1.begin() + at); std::copy(x.loss2.begin(), x.loss2.end(), l2.begin() + at); std::copy(x.loss3.begin(), x.loss3.end(), l3.begin() + at);
                std::copy(x.merged.begin(), x.merged.end(), lm.begin() + at); std::copy(x.leaving_ratio.begin(), x.leaving_ratio.end(), lr.begin() + at); std::copy(x.coming_ratio.begin(), x.coming_ratio.end(), cr.begin() + at);
                std::copy(x.leaving_count.begin(), x.leaving_count.end(), lc.begin() + at); std::copy(x.coming_count.begin(), x.coming_count.end(), cc.begin() + at);
                rd[t] = x.reads; sg[t] = x.subgraph;
            }
            at += V;
        }
        ald_batch_extras bx;
        bx.boundary_loss1 = l1.data(); bx.boundary_loss2 = l2.data(); bx.boundary_loss3 = l3.data(); bx.boundary_merged_loss = lm.data();
        bx.unbridge_leaving_count = lc.data(); bx.unbridge_leaving_ratio = lr.data(); bx.unbridge_coming_count = cc.data(); bx.unbridge_coming_ratio = cr.data();
        bx.gr_reads = rd.data(); bx.gr_subgraph = sg.data();
        const int r = ald_batch_features_all_ex(b_, &bx, feat_raw_on_device_ ? ALD_FEAT_RAW_ON_DEVICE : 0u);
        if(r != ALD_OK) throw gpu_error(r, "ald_batch_features_all_ex");
    }
    ald_batch *b_ = nullptr;
    bool feat_raw_on_device_ = false;
    std::vector<std::vector<int32_t>> lpos_, rpos_;
    std::vector<int32_t> status_;                   // per ticket, after flush_on_device()
    std::vector<graph_extras> extras_;              // per ticket, filled by the *_with_extras forms only
};

// the reference's single-graph shape: ctor + assemble() + .paths
template<class SpliceGraph, class HyperSet, class Parameters, class Path>
class gpu_scallop {
public:
    gpu_scallop(SpliceGraph &gr, HyperSet &hs, const Parameters &cfg, bool random_ordering = false, int device = 0)
        : gr_(gr), hs_(hs), batch_(cfg, device) { if(random_ordering) throw std::invalid_argument("random_ordering is not supported (always false in the reference: assembler.cc:1110)"); }
    int assemble() {
        int i = batch_.enqueue(gr_, hs_);
        batch_.flush();
        status = batch_.status(i);
        paths = batch_.paths(i);
        return 0;
    }
    // opt-in: assemble() plus the feature block of every path (the reference's update_trst_features), read from gr's own objects:
    // features[k] belongs to paths[k].  F: a type with the field names of transcript::TrstFeatures.
    template<class F>
    int assemble_with_features(std::vector<F> &features, int *features_status = nullptr) {
        int i = batch_.enqueue_with_extras(gr_, hs_);
        batch_.flush();
        status = batch_.status(i);
        paths = batch_.paths(i);
        features = batch_.template features<F>(i, features_status);
        return 0;
    }
    std::vector<Path> paths;               // scallop::paths
    int status = 0;                        // ALD_ST_*: >= 100 where the reference would have asserted
private:
    SpliceGraph &gr_; HyperSet &hs_;
    gpu_scallop_batch<SpliceGraph, HyperSet, Parameters, Path> batch_;
};

} // namespace aletsch
