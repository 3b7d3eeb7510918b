// features_raw_test.cc -- gpu_scallop_batch::features_raw_on_device (aletsch_amd/host/gpu_scallop.hpp): graphs enqueued RAW (enqueue_raw /
// enqueue_raw_with_extras, as assembler::assemble(gx, px, sid) receives them) get the same feature rows whether the host routine computes
// them (round 0, the default) or the device pass does (round 1, after features_raw_on_device(true)).  Reads graphs from stdin, prints both
// rounds' rows (doubles as their bit patterns) and how many graphs the host routine did; exit status 3 when the rounds differ.
// Driven by tests/test_features_raw_gpu.py.
//   stdin: N, then per graph "V E P reads subgraph dist", V lines "w lpos rpos loss1 loss2 loss3 merged leaving_count leaving_ratio
//          coming_count coming_ratio", E lines "s t w count" in creation order, P lines "len count coord...".  Even tickets go through
//          enqueue_raw_with_extras, odd ones through enqueue_raw (their extras read as zeros).
#include "../../aletsch_amd/host/gpu_scallop.hpp"
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <unordered_map>

struct mock_edge { int s, t; int source() const { return s; } int target() const { return t; } };
struct mock_edge_info { int strand = 0, count = 0; double abd = 0; std::set<int> samples; std::unordered_map<int, double> spAbd; };
struct mock_vertex_info { int32_t lpos = 0, rpos = 0; int type = -1; double boundary_loss1 = 0, boundary_loss2 = 0, boundary_loss3 = 0, boundary_merged_loss = 0;
                          int unbridge_leaving_count = 0; double unbridge_leaving_ratio = 0; int unbridge_coming_count = 0; double unbridge_coming_ratio = 0; };
struct mock_graph {
    std::vector<mock_edge*> es; std::vector<double> ew; std::vector<mock_edge_info> ei; std::vector<double> vw; std::vector<mock_vertex_info> vi; char strand = '.';
    int reads = 0, subgraph = 0, dist = 10000;
    size_t num_vertices() const { return vw.size(); }
    std::pair<std::vector<mock_edge*>::iterator, std::vector<mock_edge*>::iterator> edges() { return {es.begin(), es.end()}; }
    int idx(mock_edge *e) const { for(size_t i = 0; i < es.size(); i++) if(es[i] == e) return (int)i; return -1; }
    double get_edge_weight(mock_edge *e) const { return ew[idx(e)]; }
    const mock_edge_info &get_edge_info(mock_edge *e) const { return ei[idx(e)]; }
    double get_vertex_weight(int v) const { return vw[v]; }
    const mock_vertex_info &get_vertex_info(int v) const { return vi[v]; }
};
struct mock_hyper_set { std::map<std::vector<int>, int> nodes; };
struct mock_phase_set { std::map<std::vector<int32_t>, int> pmap; };
struct mock_parameters { double max_decompose_error_ratio[8] = {0.30, 0.00, 1.10, 1.10, 0.75, 0.30, 0.00, 1.00}; double min_guaranteed_edge_weight = 0.01, min_transcript_coverage = 2.0; int max_num_exons = 10000; };
struct mock_path { std::vector<int> v; std::vector<std::pair<int, int>> junc; int length = 0; double abd = 0, weight = 0, conf = 0, reads = 0; char strand = '.'; int count = 0; };
struct mock_features {                     // transcript::TrstFeatures (gtf/transcript.h:60-104), in a different member order on purpose
    double end_abd, end_weight; int end_cnt; double start_abd, start_weight; int start_cnt;
    double unbridge_end_leaving_ratio; int unbridge_end_leaving_count; double unbridge_start_coming_ratio; int unbridge_start_coming_count;
    double seq_max_ratio, seq_max_abd; int seq_max_cnt; double seq_max_wt, seq_min_ratio, seq_min_abd; int seq_min_cnt; double seq_min_wt;
    int uni_junc; double end_intron_ratio, start_intron_ratio, intron_ratio; int end_introns, start_introns, introns;
    double end_merged_loss, start_merged_loss, end_loss3, end_loss2, end_loss1, start_loss3, start_loss2, start_loss1;
    int max_mid_exon_len; double junc_ratio; int num_edges, num_vertices, gr_subgraph, gr_reads, gr_edges, gr_vertices;
};

static bool read_graph(mock_graph &g, mock_phase_set &px)
{
    int V, E, P;
    if(scanf("%d %d %d %d %d %d", &V, &E, &P, &g.reads, &g.subgraph, &g.dist) != 6) return false;
    for(int i = 0; i < V; i++) {
        double w; mock_vertex_info vi;
        if(scanf("%lf %d %d %lf %lf %lf %lf %d %lf %d %lf", &w, &vi.lpos, &vi.rpos, &vi.boundary_loss1, &vi.boundary_loss2, &vi.boundary_loss3, &vi.boundary_merged_loss,
                 &vi.unbridge_leaving_count, &vi.unbridge_leaving_ratio, &vi.unbridge_coming_count, &vi.unbridge_coming_ratio) != 11) return false;
        g.vw.push_back(w); g.vi.push_back(vi);
    }
    for(int k = 0; k < E; k++) {
        int s, t, c; double w;
        if(scanf("%d %d %lf %d", &s, &t, &w, &c) != 4) return false;
        g.es.push_back(new mock_edge{s, t}); g.ew.push_back(w); mock_edge_info ei; ei.count = c; ei.abd = w; ei.samples.insert(0); ei.spAbd[0] = w; g.ei.push_back(ei);
    }
    for(int p = 0; p < P; p++) { int len, c; if(scanf("%d %d", &len, &c) != 2) return false; std::vector<int32_t> v((size_t)len); for(int32_t &x : v) if(scanf("%d", &x) != 1) return false; px.pmap[v] += c; }
    return true;
}

static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }

static void put(std::string &out, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void put(std::string &out, const char *fmt, ...)
{
    char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap); out += buf;
}

int main()
{
    mock_parameters cfg;
    int N;
    if(scanf("%d", &N) != 1) return 2;
    std::vector<mock_graph> gs((size_t)N); std::vector<mock_phase_set> px((size_t)N);
    for(int n = 0; n < N; n++) if(!read_graph(gs[(size_t)n], px[(size_t)n])) return 2;
    std::string text[2];
    try {
        aletsch::gpu_scallop_batch<mock_graph, mock_hyper_set, mock_parameters, mock_path> batch(cfg, 0);
        for(int round = 0; round < 2; round++) {                       // round 0: raw graphs by the host routine; round 1: by the device pass
            batch.features_raw_on_device(round == 1);
            std::vector<int> t;
            for(int n = 0; n < N; n++) t.push_back(n % 2 == 0 ? batch.enqueue_raw_with_extras(gs[(size_t)n], px[(size_t)n], gs[(size_t)n].dist) : batch.enqueue_raw(gs[(size_t)n], px[(size_t)n], gs[(size_t)n].dist));
            batch.flush();
            std::string &out = text[round];
            for(int n = 0; n < N; n++) {
                int st = -1; std::vector<int> comp;
                std::vector<mock_features> f = batch.features<mock_features>(t[(size_t)n], &st, &comp);
                put(out, "graph %d rc %d rows %d\n", n, st, (int)f.size());
                for(size_t k = 0; k < f.size(); k++) {
                    const mock_features &x = f[k];
                    put(out, "%d %d %d %d %d %d %d %016llx %d", comp[k], x.gr_vertices, x.gr_edges, x.gr_reads, x.gr_subgraph, x.num_vertices, x.num_edges, bits(x.junc_ratio), x.max_mid_exon_len);
                    const double d1[] = {x.start_loss1, x.start_loss2, x.start_loss3, x.end_loss1, x.end_loss2, x.end_loss3, x.start_merged_loss, x.end_merged_loss};
                    for(double d : d1) put(out, " %016llx", bits(d));
                    put(out, " %d %d %d %016llx %016llx %016llx %d", x.introns, x.start_introns, x.end_introns, bits(x.intron_ratio), bits(x.start_intron_ratio), bits(x.end_intron_ratio), x.uni_junc);
                    put(out, " %016llx %d %016llx %016llx %016llx %d %016llx %016llx", bits(x.seq_min_wt), x.seq_min_cnt, bits(x.seq_min_abd), bits(x.seq_min_ratio), bits(x.seq_max_wt), x.seq_max_cnt, bits(x.seq_max_abd), bits(x.seq_max_ratio));
                    put(out, " %d %016llx %d %016llx", x.unbridge_start_coming_count, bits(x.unbridge_start_coming_ratio), x.unbridge_end_leaving_count, bits(x.unbridge_end_leaving_ratio));
                    put(out, " %d %016llx %016llx %d %016llx %016llx\n", x.start_cnt, bits(x.start_weight), bits(x.start_abd), x.end_cnt, bits(x.end_weight), bits(x.end_abd));
                }
            }
            int64_t dev = -1, host = -1;
            if(ald_batch_features_stats(batch.handle(), nullptr, nullptr, &dev, &host) != ALD_OK) return 2;
            printf("round %d device_graphs %lld host_graphs %lld\n%s", round, (long long)dev, (long long)host, out.c_str());
            batch.clear();
        }
    } catch(const std::exception &e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    if(text[0] != text[1]) { fprintf(stderr, "the rows of the two rounds differ\n"); return 3; }
    return 0;
}
