// mock_types.h -- TEST-ONLY: mock types that carry the member names of the reference's splice_graph / hyper_set / phase_set / parameters
// (what aletsch::gpu_assembly_queue is instantiated with in dispatch_test.cc and queue_tsan_main.cc), and the reader of the text form
// tests/test_gpu_adapter.py::graph_text writes: "V E P", V lines "weight lpos rpos", E lines "source target weight" in creation order,
// P lines "len count v0 v1 ..." (phasing lists; for a raw graph the same lines hold a phase in exon coordinates).
#pragma once
#include "../../aletsch_amd/host/gpu_dispatch.hpp"
#include <cstdio>
#include <cstdint>
#include <set>
#include <unordered_map>

struct mock_edge { int s, t, id; int source() const { return s; } int target() const { return t; } };
struct mock_edge_info { int strand = 0, count = 0; double abd = 0; std::set<int> samples; std::unordered_map<int, double> spAbd; };
struct mock_vertex_info { int32_t lpos = 0, rpos = 0; int type = -1; };
struct mock_graph {
    std::vector<mock_edge*> es; std::vector<double> ew; std::vector<mock_edge_info> ei; std::vector<double> vw; std::vector<mock_vertex_info> vi; char strand = '.';
    size_t num_vertices() const { return vw.size(); }
    std::pair<std::vector<mock_edge*>::iterator, std::vector<mock_edge*>::iterator> edges() { return {es.begin(), es.end()}; }
    double get_edge_weight(const mock_edge *e) const { return ew[(size_t)e->id]; }
    const mock_edge_info &get_edge_info(const mock_edge *e) const { return ei[(size_t)e->id]; }
    double get_vertex_weight(int v) const { return vw[(size_t)v]; }
    const mock_vertex_info &get_vertex_info(int v) const { return vi[(size_t)v]; }
};
struct mock_hyper_set { std::map<std::vector<int>, int> nodes; };
struct mock_parameters { double max_decompose_error_ratio[8] = {0.30, 0.00, 1.10, 1.10, 0.75, 0.30, 0.00, 1.00}; double min_guaranteed_edge_weight = 0.01, min_transcript_coverage = 2.0; int max_num_exons = 10000; };
struct mock_phase_set { std::map<std::vector<int32_t>, int> pmap; };

// one graph from `in`; false at a malformed or truncated record
inline bool read_mock_graph(FILE *in, mock_graph &g, mock_hyper_set &hs)
{
    int V, E, P;
    if(fscanf(in, "%d %d %d", &V, &E, &P) != 3) return false;
    for(int i = 0; i < V; i++) { double w; int l, r; if(fscanf(in, "%lf %d %d", &w, &l, &r) != 3) return false; g.vw.push_back(w); mock_vertex_info vi; vi.lpos = l; vi.rpos = r; g.vi.push_back(vi); }
    for(int k = 0; k < E; k++) { int s, t; double w; if(fscanf(in, "%d %d %lf", &s, &t, &w) != 3) return false; g.es.push_back(new mock_edge{s, t, k}); g.ew.push_back(w); mock_edge_info ei; ei.count = 1; ei.abd = w; ei.samples.insert(0); ei.spAbd[0] = w; g.ei.push_back(ei); }
    for(int p = 0; p < P; p++) { int len, c; if(fscanf(in, "%d %d", &len, &c) != 2) return false; std::vector<int> v((size_t)len); for(int &x : v) if(fscanf(in, "%d", &x) != 1) return false; hs.nodes[v] += c; }
    return true;
}
