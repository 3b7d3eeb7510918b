// compact_input_cases.h -- the ONE case list of the compact-input tests: the smallest shapes at which a step of the device-side expansion
// (aletsch_amd/csrc/input_expand.h) or its host bookkeeping (HostBatch: layout's `derived` marks, ensure_in_csr, the def_* / uni_samples
// flags) can go wrong.  Read by tests/compact_input_main.cc (CPU tier: g++, sanitizers, host_pack.h only) and by
// tests/compact_input_gpu_main.hip (GPU tier: the same batches through the kernels, byte comparison of every section).
//
// A case is a list of GROUPS; a group is staged by one add_packed_raw call ("packed" staging) or graph by graph through add_graph /
// add_graph_raw ("single" staging).  `expect` is the set of sections layout() must mark derived in compact mode.
#pragma once
#include "../aletsch_amd/csrc/host_pack.h"
#include <cmath>
#include <string>
#include <utility>
#include <vector>

namespace cic {
using namespace ald;

struct G {
    int V = 0;
    std::vector<int32_t> voff, tgt, esoff, sid, lpos, rpos; std::vector<double> ew, sabd, vw;
    std::vector<double> eabd; std::vector<int32_t> ecount, vtype, rank; std::vector<uint8_t> estrand;      // optional columns: with_* says whether the caller supplies them
    bool with_eabd = false, with_ecount = false, with_vtype = false, with_estrand = false, with_rank = false;
    std::vector<int32_t> poff{0}, pv, pc;                  // phasing lists (a staged graph only)
    int raw_dist = -1;                                     // >= 0: a raw graph, with these phases
    std::vector<int32_t> rpoff{0}, rpcoord, rpcount;
    int E() const { return (int)tgt.size(); }
    int P() const { return (int)pc.size(); }
};
typedef std::vector<std::pair<int, int>> Edges;

// edges (s, t), s < t, in any order -> CSR rows sorted by (source, target); one sample `sid` per edge whose abundance is the weight
inline G make(int V, Edges e, int sid = 0)
{
    std::stable_sort(e.begin(), e.end());
    G g; g.V = V; g.voff.assign((size_t)V + 1, 0);
    for(auto &x : e) g.voff[(size_t)x.first + 1]++;
    for(int i = 0; i < V; i++) g.voff[(size_t)i + 1] += g.voff[(size_t)i];
    g.esoff.push_back(0);
    for(size_t k = 0; k < e.size(); k++) {
        const double w = 2.0 + 0.25 * (double)((k * 7 + (size_t)e[k].first) % 11);
        g.tgt.push_back(e[k].second); g.ew.push_back(w); g.sid.push_back(sid); g.sabd.push_back(w); g.esoff.push_back((int32_t)k + 1);
    }
    for(int i = 0; i < V; i++) { g.vw.push_back(1.0 + i); g.lpos.push_back(100 * i); g.rpos.push_back(100 * i + 50); }
    return g;
}
inline G chain(int V, int skip_every = 0, int sid = 0)     // 0 -> 1 -> ... -> V-1, plus i -> i + 2 from every skip_every-th vertex
{
    Edges e; for(int i = 0; i + 1 < V; i++) e.push_back({i, i + 1});
    if(skip_every > 0) for(int i = 0; i + 2 < V; i += skip_every) e.push_back({i, i + 2});
    return make(V, e, sid);
}
inline G in_fan(int n, int sid = 0)                         // source -> n vertices -> one hub -> sink: an in-list of n
{
    Edges e; const int hub = n + 1;
    for(int i = 1; i <= n; i++) { e.push_back({0, i}); e.push_back({i, hub}); }
    e.push_back({hub, hub + 1});
    return make(n + 3, e, sid);
}
inline G dag(int V, int E, unsigned seed, int sid = 0)      // E edges s < t drawn by a small generator (parallel edges happen)
{
    Edges e; unsigned x = seed * 2654435761u + 12345u;
    for(int k = 0; k < E; k++) { x = x * 1664525u + 1013904223u; const int s = (int)((x >> 8) % (unsigned)(V - 1)); x = x * 1664525u + 1013904223u; const int t = s + 1 + (int)((x >> 8) % (unsigned)(V - 1 - s)); e.push_back({s, t}); }
    return make(V, e, sid);
}
// replaces the sample lists: one list of (id, abundance) per edge
inline void set_samples(G &g, const std::vector<std::vector<std::pair<int, double>>> &lists)
{
    g.esoff.assign(1, 0); g.sid.clear(); g.sabd.clear();
    for(auto &l : lists) { for(auto &s : l) { g.sid.push_back(s.first); g.sabd.push_back(s.second); } g.esoff.push_back((int32_t)g.sid.size()); }
}
inline G with_abd_count(G g) { g.with_eabd = g.with_ecount = true; for(int k = 0; k < g.E(); k++) { g.eabd.push_back(0.5 + k); g.ecount.push_back(2 + k % 3); } return g; }
inline G with_type_strand(G g) { g.with_vtype = g.with_estrand = true; for(int i = 0; i < g.V; i++) g.vtype.push_back(i % 3 - 1); for(int k = 0; k < g.E(); k++) g.estrand.push_back((uint8_t)(k % 3)); return g; }
inline G raw(G g, int dist, bool phase) { g.raw_dist = dist; if(phase && g.V >= 4) { g.rpcoord = {g.lpos[1], g.rpos[1], g.lpos[2], g.rpos[2]}; g.rpoff = {0, 4}; g.rpcount = {3}; } return g; }

struct Case { std::string name; std::vector<std::vector<G>> groups; unsigned expect; };
enum { D_ALL = ALD_DERIVE_INCSR | ALD_DERIVE_SAMPLES | ALD_DERIVE_EABD | ALD_DERIVE_ECOUNT | ALD_DERIVE_VTYPE | ALD_DERIVE_ESTRAND,
       D_NO_SAMPLES = D_ALL & ~ALD_DERIVE_SAMPLES };

inline std::vector<G> uniform_batch() { return {dag(12, 30, 1, 5), chain(6, 2, 9), in_fan(4, 0)}; }

inline std::vector<Case> cases()
{
    std::vector<Case> c;
    c.push_back({"v2_e0", {{make(2, {})}}, D_ALL});
    c.push_back({"one_source_sink_edge", {{make(2, {{0, 1}})}}, D_ALL});
    c.push_back({"three_parallel_source_sink_edges", {{make(2, {{0, 1}, {0, 1}, {0, 1}})}}, D_ALL});
    c.push_back({"chain_of_5", {{chain(5)}}, D_ALL});
    for(int n : {1, 63, 64, 65, 300}) c.push_back({"in_fan_" + std::to_string(n), {{in_fan(n)}}, D_ALL});
    { G g = make(4, {{0, 1}, {1, 2}, {1, 2}, {1, 2}, {2, 3}}); g.with_rank = true; g.rank = {0, 3, 2, 1, 4};      // the in-CSR orders by id, not by rank
      c.push_back({"parallel_mid_edges_reversed_rank", {{g}}, D_ALL}); }
    for(int e : {63, 64, 65, 127, 128, 129}) c.push_back({"edges_" + std::to_string(e), {{dag(20, e, (unsigned)e)}}, D_ALL});
    c.push_back({"three_graphs_first_without_edges", {{make(2, {}), chain(5, 0, 3), in_fan(3, 4)}}, D_ALL});      // the + g in the offset index
    // the kernels have ONE form for every size (no threshold between two paths); what changes with V is the number of 64-entry steps of
    // the scan over the V + 1 counters: 1024 of them end a step exactly, 1025 begin another
    c.push_back({"v1023_scan_ends_on_a_step", {{chain(1023, 3)}}, D_ALL});
    c.push_back({"v1024_scan_one_past_a_step", {{chain(1024, 3)}}, D_ALL});
    c.push_back({"v10241_beyond_every_class", {{chain(10241, 2)}}, D_ALL});
    c.push_back({"large_and_small_in_one_batch", {{chain(1024, 2, 1), in_fan(65, 2), chain(1023, 2, 3), make(2, {})}}, D_ALL});
    { G g = chain(6);                                      // edges with 0, 1 and 3 samples; -0.0 alone sums to +0.0; a sum that depends on the order
      set_samples(g, {{}, {{2, -0.0}}, {{1, 1e16}, {4, 1.0}, {7, -1e16}}, {{3, 2.5}}, {{0, 1.0}, {1, 2.0}, {2, 3.0}}});
      c.push_back({"samples_0_1_3_negative_zero_order", {{g}}, D_NO_SAMPLES}); }
    { G g = chain(4); set_samples(g, {{{5, 1.0}, {2, 1e16}, {3, -1e16}}, {{1, 2.0}}, {{1, 3.0}}});                // descending ids: staging sorts the list, the default
      c.push_back({"unsorted_sample_list", {{g}}, D_NO_SAMPLES & ~ALD_DERIVE_EABD}); }                            // edge_abd was summed in the caller's order and has to travel
    // C: the sample lists
    c.push_back({"uniform_batch", {uniform_batch()}, D_ALL});
    { auto b = uniform_batch(); b[1].sabd[2] = std::nextafter(b[1].sabd[2], 1e300); c.push_back({"uniform_but_one_abundance_off_by_an_ulp", {b}, D_NO_SAMPLES}); }
    { auto b = uniform_batch(); b[0].sid[7] = 6; c.push_back({"uniform_but_one_sample_id", {b}, D_NO_SAMPLES}); }
    { auto b = uniform_batch(); G &g = b[2]; const int E = g.E();                                                  // an edge of 0 samples, then one of 2: the totals still agree
      std::vector<std::vector<std::pair<int, double>>> l; for(int k = 0; k < E; k++) l.push_back({{0, g.ew[(size_t)k]}});
      l[1].clear(); l[2] = {{0, g.ew[2]}, {1, g.ew[2]}}; set_samples(g, l);
      c.push_back({"uniform_but_0_then_2_samples", {b}, D_NO_SAMPLES}); }
    // B: the defaults, each on its own; B and C are independent
    c.push_back({"one_graph_supplies_abd_and_count", {{with_abd_count(dag(10, 20, 7, 1))}, {dag(9, 15, 8, 2)}}, D_ALL & ~(ALD_DERIVE_EABD | ALD_DERIVE_ECOUNT)});
    c.push_back({"one_graph_supplies_type_and_strand", {{dag(9, 15, 8, 2)}, {with_type_strand(chain(7, 2, 3))}}, D_ALL & ~(ALD_DERIVE_VTYPE | ALD_DERIVE_ESTRAND)});
    // raw graphs mixed with staged ones (a staged one with phasing lists)
    { G s = chain(6, 2, 1); s.pv = {1, 2, 3, 2, 4}; s.poff = {0, 3, 5}; s.pc = {2, 1};
      c.push_back({"raw_mixed_with_staged", {{raw(chain(6, 3, 2), 10000, true), s, raw(in_fan(3, 0), 50, false)}, {chain(5)}}, D_ALL}); }
    return c;
}

// ---- staging ----
inline int stage_single(HostBatch &B, const G &g)
{
    ald_graph_view v; memset(&v, 0, sizeof(v)); static const int32_t zi = 0; static const double zd = 0;
    v.num_vertices = g.V; v.num_edges = g.E(); v.num_phasing = g.raw_dist >= 0 ? 0 : g.P();
    v.vertex_offset = g.voff.data(); v.edge_target = g.E() ? g.tgt.data() : &zi; v.edge_weight = g.E() ? g.ew.data() : &zd; v.edge_sample_offset = g.esoff.data();
    v.sample_id = g.sid.empty() ? &zi : g.sid.data(); v.sample_abd = g.sabd.empty() ? &zd : g.sabd.data();
    v.edge_strand = g.with_estrand ? g.estrand.data() : nullptr; v.edge_abd = g.with_eabd ? g.eabd.data() : nullptr; v.edge_count = g.with_ecount ? g.ecount.data() : nullptr;
    v.vertex_weight = g.vw.data(); v.vertex_lpos = g.lpos.data(); v.vertex_rpos = g.rpos.data(); v.vertex_type = g.with_vtype ? g.vtype.data() : nullptr;
    v.phasing_offset = g.poff.data(); v.phasing_vertex = g.pv.empty() ? &zi : g.pv.data(); v.phasing_count = g.pc.empty() ? &zi : g.pc.data();
    v.strand = '.'; v.edge_creation_rank = g.with_rank ? g.rank.data() : nullptr;
    if(g.raw_dist < 0) return B.add_graph(v);
    ald_phase_view ph; memset(&ph, 0, sizeof(ph));
    ph.num_phases = (int32_t)g.rpcount.size(); ph.phase_offset = g.rpoff.data(); ph.phase_coord = g.rpcoord.empty() ? &zi : g.rpcoord.data(); ph.phase_count = g.rpcount.empty() ? &zi : g.rpcount.data();
    return B.add_graph_raw(v, &ph, g.raw_dist);
}
// one add_packed_raw call for the whole group (the optional columns of a group are those of its first graph)
inline int stage_packed(HostBatch &B, const std::vector<G> &grp)
{
    std::vector<int32_t> nv, ne, np, voff, tgt, esoff, sid, lpos, rpos, ecount, vtype, rank, poff, pv, pc, rdist, nph, rpoff, rpcoord, rpcount; std::vector<double> ew, sabd, vw, eabd; std::vector<uint8_t> estrand;
    auto cat = [](auto &d, const auto &s) { d.insert(d.end(), s.begin(), s.end()); };
    bool any_raw = false; const G &f = grp[0];
    for(const G &g : grp) {
        const bool is_raw = g.raw_dist >= 0; any_raw = any_raw || is_raw;
        nv.push_back(g.V); ne.push_back(g.E()); np.push_back(is_raw ? 0 : g.P());
        cat(voff, g.voff); cat(tgt, g.tgt); cat(ew, g.ew); cat(esoff, g.esoff); cat(sid, g.sid); cat(sabd, g.sabd); cat(vw, g.vw); cat(lpos, g.lpos); cat(rpos, g.rpos);
        if(f.with_eabd) cat(eabd, g.eabd);
        if(f.with_ecount) cat(ecount, g.ecount);
        if(f.with_vtype) cat(vtype, g.vtype);
        if(f.with_estrand) cat(estrand, g.estrand);
        if(f.with_rank) cat(rank, g.rank);
        if(is_raw) { poff.push_back(0); nph.push_back((int32_t)g.rpcount.size()); cat(rpoff, g.rpoff); cat(rpcoord, g.rpcoord); cat(rpcount, g.rpcount); }
        else { cat(poff, g.poff); cat(pv, g.pv); cat(pc, g.pc); nph.push_back(0); rpoff.push_back(0); }
        rdist.push_back(g.raw_dist);
    }
    for(auto *x : {&tgt, &sid, &pv, &pc, &rpcoord, &rpcount}) x->push_back(0);      // never a null pointer for an empty column
    ew.push_back(0); sabd.push_back(0);
    return B.add_packed_raw((int32_t)grp.size(), nv.data(), ne.data(), np.data(), voff.data(), tgt.data(), ew.data(), f.with_estrand ? estrand.data() : nullptr, f.with_eabd ? eabd.data() : nullptr,
                            esoff.data(), sid.data(), sabd.data(), vw.data(), lpos.data(), rpos.data(), f.with_vtype ? vtype.data() : nullptr, poff.data(), pv.data(), pc.data(), nullptr,
                            f.with_ecount ? ecount.data() : nullptr, f.with_rank ? rank.data() : nullptr, any_raw ? rdist.data() : nullptr, nph.data(), rpoff.data(), rpcoord.data(), rpcount.data());
}
inline int stage(HostBatch &B, const Case &c, bool packed)
{
    for(auto &grp : c.groups) {
        if(packed) { const int rc = stage_packed(B, grp); if(rc != ALD_OK) return rc; }
        else for(auto &g : grp) { const int rc = stage_single(B, g); if(rc != ALD_OK) return rc; }
    }
    return ALD_OK;
}
inline const char *section_name(int i)
{
    static const char *n[HostBatch::S_COUNT] = {"NV", "NE", "NP", "OFFV", "OFFE", "OFFS", "OFFP", "OFFPV", "VOFF", "ETGT", "EW", "ESTRAND", "EABD", "ESOFF", "SID", "SABD", "VW", "LPOS", "RPOS", "VTYPE",
                                                "INOFF", "INEDGE", "POFF", "PV", "PC", "GSTRAND", "ECOUNT", "ERANK", "RAWDIST", "OFFRP", "OFFRC", "RPOFF", "RPCOORD", "RPCOUNT"};
    return n[i];
}

} // namespace cic
