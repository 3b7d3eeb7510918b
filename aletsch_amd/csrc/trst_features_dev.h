// trst_features_dev.h -- the per-graph routine of the batched feature pass (trst_features.hip): scallop::update_trst_features
// (scallop/scallop.cc:3268-3451) + unique_junc (:3472-3497) for every path of ONE staged graph, by one wave.  Written with the macros of
// decomp_common.h, so that tests/feature_emu compiles the same routine with g++ (-DALD_EMU, one lane) against the oracle.
//
// What it reads is what a downloaded batch holds in HBM: the staged graph (wire sections of d_in, in-CSR included), the path records
// (d_pool) named by the result index the decomposition kernel wrote (index[graph_first[g] + p]; the pool also holds records of abandoned
// capacity attempts, which the index never names), and the extras of the caller.  The semantics are those of the host routine
// ald_batch_features (trst_features.cpp), expression for expression, so the rows are equal bit for bit:
//   * edge(s, t) is the NEWEST parallel edge: the last match in the out-row, which is sorted by (target, creation);
//   * get_in_weights / get_out_weights add in adjacency order (in-CSR order / out-row order), one addition after the other;
//   * std::min / std::max are written out as the ternaries the library defines them by (NaN handling included);
//   * the file is compiled with -ffp-contract=off: no FMA where the reference has none.
//
// Work split: lanes over the paths of the graph.  First the junction list of every path (path::junc, scallop.cc:2812-2820) is written
// to LDS -- or, for a graph whose lists cannot fit there, to a scratch buffer with two words per word of the record pool, at the
// record's own offset --, then every lane computes the rows of its paths against the lists of all others, exactly as the host loop does.
//
// Raw graphs (FeatArgs::g_ew set; ald_batch_features_all_ex with ALD_FEAT_RAW_ON_DEVICE).  Of the pre-steps of assemble(gx, px, sid) only
// group_start_boundaries / group_end_boundaries (rnacore/graph_reviser.cc:916-1066) change what the features read: the source / sink edges
// of folded boundaries die, the leader edge and the chain edges j -> j+1 take on weight (and, on the start side, count).  The wire rows of
// a raw graph are already sorted by (target, creation) and are never modified, so the grouped graph is the wire graph plus an OVERLAY per
// edge -- weight, count, a dead flag -- which the wave builds first (ft_group_boundaries: pre_assemble_device of decomp_device.h without
// vertex weights, strands, boundary maps, phases and rank compaction).  The live edges keep the relative order the host's re-staging gives
// them, so every sum adds in the same order.  Raw-ness is a template parameter: the staged instantiation never tests a dead flag.
#pragma once
#include "decomp_common.h"

namespace ald {

enum { FT_LDS_WORDS = 4096 };          // per wave (16 KB): (offset, count) per path, then the junction pairs

struct FeatArgs {
    BatchIn in;                                          // the staged graphs (wire sections)
    ALD_GLOBAL const uint32_t *pool;                     // path records
    ALD_GLOBAL const unsigned long long *index;          // index[graph_first[g] + p] = pool offset of record (g, p)
    ALD_GLOBAL const long long *graph_first;             // [n]
    ALD_GLOBAL const int32_t *n_paths;                   // [n] 0 for a graph that did not end OK / SKIPPED_LARGE
    ALD_GLOBAL const int64_t *row_begin;                 // [n+1] first row of every graph (paths in (graph, path) order)
    // extras (ald_batch_extras): [sum V] at off_v[g] + v, [n] per graph; null = zeros
    ALD_GLOBAL const double *loss1, *loss2, *loss3, *merged_loss;
    ALD_GLOBAL const int32_t *leaving_count; ALD_GLOBAL const double *leaving_ratio;
    ALD_GLOBAL const int32_t *coming_count;  ALD_GLOBAL const double *coming_ratio;
    ALD_GLOBAL const int32_t *gr_reads, *gr_subgraph;
    int32_t *scratch;                                    // 2 words per pool word, or null when every graph fits LDS
    int32_t lds_words;                                   // LDS budget of this launch (FT_LDS_WORDS; 0 sends every graph to the scratch)
    int32_t pad;
    ALD_GLOBAL ald_trst_features *rows;                  // [total paths]
    ALD_GLOBAL int32_t *complete;                        // [total paths]
    ALD_GLOBAL int32_t *graph_rc;                        // [n] what ald_batch_features returns for the graph
    // the grouped-graph overlay of raw graphs, written by the wave of the graph before it reads it: per edge of the BATCH at off_e[g] + k
    // (staged graphs leave their stretch untouched), live edges per graph [n].  All null: raw graphs are left to the host routine.
    ALD_GLOBAL double *g_ew; ALD_GLOBAL int32_t *g_ecount; ALD_GLOBAL uint8_t *g_dead; ALD_GLOBAL int32_t *g_live;
};

// one staged graph as the features read it (host routine: GraphRO)
struct FtGraph {
    ALD_GLOBAL const int32_t *voff, *etgt, *ecount, *lpos, *rpos, *ioff, *iedge;
    ALD_GLOBAL const double *ew, *eabd;
    ALD_GLOBAL const uint8_t *dead;                      // raw graphs only: edges the boundary grouping removed (ew / ecount then point at the overlay)
    int64_t ov; int V, E;
};

template<bool RAW> ALD_INL int ft_edge(const FtGraph &G, int s, int t)           // newest (RAW: live) parallel edge s -> t, or -1
{
    if(s < 0 || s >= G.V) return -1;
    int best = -1;
    for(int k = G.voff[s]; k < G.voff[s + 1]; k++) { if(RAW && G.dead[k]) continue; const int tt = G.etgt[k]; if(tt == t) best = k; else if(tt > t) break; }
    return best;
}
template<bool RAW> ALD_INL double ft_out_weights(const FtGraph &G, int v) { double s = 0; for(int k = G.voff[v]; k < G.voff[v + 1]; k++) { if(RAW && G.dead[k]) continue; s += G.ew[k]; } return s; }
template<bool RAW> ALD_INL double ft_in_weights(const FtGraph &G, int v) { double s = 0; for(int k = G.ioff[v]; k < G.ioff[v + 1]; k++) { const int e = G.iedge[k]; if(RAW && G.dead[e]) continue; s += G.ew[e]; } return s; }
ALD_INL double ft_dmin(double a, double b) { return b < a ? b : a; }                  // std::min
ALD_INL double ft_dmax(double a, double b) { return a < b ? b : a; }                  // std::max
ALD_INL int ft_imin(int a, int b) { return b < a ? b : a; }
ALD_INL int ft_imax(int a, int b) { return a < b ? b : a; }
ALD_INL double ft_dx(ALD_GLOBAL const double *a, int64_t i) { return a ? a[i] : 0.0; }
ALD_INL int ft_ix(ALD_GLOBAL const int32_t *a, int64_t i) { return a ? a[i] : 0; }

// the junction list of path p: pairs (first, second) at the returned pointer, nj of them
ALD_INL int32_t *ft_junc(const FeatArgs &A, int32_t *lds, bool in_lds, int np, long long gf, int p, int &nj)
{
    if(in_lds) { nj = lds[2 * p + 1]; return lds + 2 * np + lds[2 * p]; }
    const unsigned long long o = A.index[gf + p];
    nj = A.scratch[2 * o];
    return A.scratch + 2 * (o + ALD_REC_HDR);
}

// ratio_of of the host routine: the junction weight over the smaller of the two flanking within-exon edges; a missing edge is the assert
template<bool RAW> ALD_INL void ft_ratio_of(const FtGraph &G, int qa, int qb, double &dst, bool &bad)
{
    const int e = ft_edge<RAW>(G, qa, qb), e1 = ft_edge<RAW>(G, qa, qa + 1), e2 = ft_edge<RAW>(G, qb - 1, qb);
    if(e < 0 || e1 < 0 || e2 < 0) { bad = true; return; }
    const double r = G.ew[e] / ft_dmin(G.ew[e1], G.ew[e2]);
    if(dst < r) dst = r;
}

// ---- raw graphs: the boundary grouping on the overlay, by ONE lane (the source's and the sink's rows are short).  G reads the wire for
// adjacency and coordinates and the overlay (gw / gc / gd, already a copy of the wire's weights and counts, no edge dead) for the rest.
ALD_INL bool ft_continuous(const FtGraph &G, int x, int y)      // check_continuous_vertices (essential.cc:436-446) on the live edges
{
    for(int i = x; i < y; i++) { if(ft_edge<true>(G, i, i + 1) < 0) return false; if(G.rpos[i] != G.lpos[i + 1]) return false; }
    return true;
}
ALD_INL int ft_source(const FtGraph &G, int e)                  // the vertex whose out-row holds edge e: the last s with voff[s] <= e
{
    int lo = 0, hi = G.V - 1;
    while(lo < hi) { const int mid = (lo + hi + 1) >> 1; if(G.voff[mid] <= e) lo = mid; else hi = mid - 1; }
    return lo;
}
// group_start_boundaries / group_end_boundaries (graph_reviser.cc:916-1066) as pre_assemble_device (decomp_device.h) and ald_pre_assemble
// (pre_steps.cpp) restate them; returns the number of edges that died, or -1 where the reference would have asserted
ALD_INL int ft_group_boundaries(const FtGraph &G, int dist, ALD_GLOBAL double *gw, ALD_GLOBAL int32_t *gc, ALD_GLOBAL uint8_t *gd)
{
    int removed = 0;
    {   // start boundaries that reach the same run of touching vertices within `dist` fold into the leftmost one: weight AND count move
        const int r0 = G.voff[0], r1 = G.voff[1];                    // the source's row: targets ascending (parallel ones were refused at staging)
        if(r1 - r0 > 1) {
            const int v0 = G.etgt[r0]; int32_t p2 = G.lpos[v0]; int k1 = v0, k2 = v0, pa = r0;
            for(int q = r0 + 1; q < r1; q++) {
                const int vi = G.etgt[q]; const int32_t p = G.lpos[vi];
                const double wb = gw[q]; const int cb = gc[q];
                bool b = ft_continuous(G, k2, vi);
                if(p < p2) return -1;                                  // assert(p >= p2)
                if(p - p2 > dist) b = false;
                if(!b) { p2 = p; k1 = vi; k2 = vi; pa = q; continue; }
                for(int j = k1; j < vi; j++) {
                    const int pc = ft_edge<true>(G, j, j + 1);
                    if(pc < 0) return -1;                              // assert(pc.second == true)
                    gc[pc] += cb; gw[pc] = gw[pc] + wb;
                }
                gw[pa] += wb; gc[pa] += cb;
                gd[q] = 1; removed++;
                k2 = vi; p2 = p;
            }
        }
    }
    {   // the mirror image over the sink's live in-edges, from the right -- with the reference's own asymmetries: no count moves
        const int n = G.V - 1, i0 = G.ioff[n], i1 = G.ioff[n + 1];    // in-edges of the sink: sources ascending
        int q = i1 - 1; while(q >= i0 && gd[G.iedge[q]]) q--;
        if(q >= i0) {
            int pa = G.iedge[q]; const int v0 = ft_source(G, pa); int32_t p2 = G.rpos[v0]; int k1 = v0, k2 = v0;
            for(q--; q >= i0; q--) {
                const int pb = G.iedge[q]; if(gd[pb]) continue;
                const int vi = ft_source(G, pb); const int32_t p = G.rpos[vi]; const double wb = gw[pb];
                bool b = ft_continuous(G, vi, k2);
                if(p > p2) return -1;                                  // assert(p <= p2)
                if(p2 - p > dist) b = false;
                if(!b) { p2 = p; k1 = vi; k2 = vi; pa = pb; continue; }
                for(int j = vi; j < k1; j++) {
                    const int pc = ft_edge<true>(G, j, j + 1);
                    if(pc < 0) return -1;
                    const double wc = gw[pc]; gw[pc] = wc + wb;
                }
                gw[pa] += wb;
                gd[pb] = 1; removed++;
                k2 = vi; p2 = p;
            }
        }
    }
    return removed;
}

// every row of graph g; lds: FT_LDS_WORDS words private to the wave (any memory in the emulation)
template<bool RAW> ALD_INL void features_graph_t(const FeatArgs &A, int g, int32_t *lds)
{
    const int lane = lane_id();
    const BatchIn &in = A.in;
    const int np = A.n_paths[g];
    if(np <= 0) { if(lane == 0) A.graph_rc[g] = ALD_OK; return; }
    const long long gf = A.graph_first[g];
    const int64_t r0 = A.row_begin[g];
    FtGraph G;
    { const int64_t ov = in.off_v[g], ovo = ov + g, oe = in.off_e[g];
      G.voff = in.vertex_offset + ovo; G.ioff = in.in_offset + ovo; G.etgt = in.edge_target + oe; G.iedge = in.in_edge + oe; G.ecount = in.edge_count + oe;
      G.ew = in.edge_weight + oe; G.eabd = in.edge_abd + oe; G.lpos = in.vertex_lpos + ov; G.rpos = in.vertex_rpos + ov; G.ov = ov; G.V = in.g_nv[g]; G.E = in.g_ne[g]; }
    if(RAW) {
        // ---- the grouped graph: the overlay starts as a copy of the wire's weights and counts with no edge dead, lane 0 folds the boundaries
        const int64_t oe = in.off_e[g]; const int E0 = G.E;
        ALD_GLOBAL double *gw = A.g_ew + oe; ALD_GLOBAL int32_t *gc = A.g_ecount + oe; ALD_GLOBAL uint8_t *gd = A.g_dead + oe;
        for(int k = lane; k < E0; k += ALD_WAVE) { gw[k] = G.ew[k]; gc[k] = G.ecount[k]; gd[k] = 0; }
        G.ew = gw; G.ecount = gc; G.dead = gd;
        wsync_mem();
        int live = 0;
        if(lane == 0) { const int removed = ft_group_boundaries(G, in.g_rawdist[g], gw, gc, gd); live = removed < 0 ? -1 : E0 - removed; A.g_live[g] = live; }
        live = wshfl(live, 0);
        wsync_mem();
        if(live < 0) {                                                // the reference would have asserted in the grouping: as the host routine, no row is computed
            const ald_trst_features Z = {};
            for(int p = lane; p < np; p += ALD_WAVE) { A.rows[r0 + p] = Z; A.complete[r0 + p] = 0; }
            if(lane == 0) A.graph_rc[g] = ALD_ST_INVARIANT + ALD_INV_OTHER;
            return;
        }
        G.E = live;                                                   // what gr_edges reports
    }

    // ---- where the junction lists go: LDS when (offset, count) per path + the most junctions every path can have fit
    int bound = 0;
    for(int p = lane; p < np; p += ALD_WAVE) { const int nv = (int)A.pool[A.index[gf + p] + ALD_REC_NV]; bound += nv > 3 ? nv - 3 : 0; }
    for(int off = ALD_WAVE / 2; off >= 1; off >>= 1) bound += wshfl(bound, lane ^ off);
    const bool in_lds = (int64_t)2 * np + 2 * (int64_t)bound <= (int64_t)A.lds_words;
    if(!in_lds && !A.scratch) { if(lane == 0) A.graph_rc[g] = ALD_ERR_NOMEM; return; }    // (the host sizes the scratch so that this is never taken)
    if(in_lds && lane == 0) {
        int acc = 0;
        for(int p = 0; p < np; p++) { lds[2 * p] = 2 * acc; const int nv = (int)A.pool[A.index[gf + p] + ALD_REC_NV]; acc += nv > 3 ? nv - 3 : 0; }
    }
    wsync();
    // ---- path::junc: consecutive INTERNAL vertices that do not touch.  A vertex outside the graph (never written by the kernel) makes the
    // path's list empty; its row then reports the assert below.
    for(int p = lane; p < np; p += ALD_WAVE) {
        const unsigned long long o = A.index[gf + p];
        ALD_GLOBAL const uint32_t *pv = A.pool + o + ALD_REC_HDR; const int n = (int)A.pool[o + ALD_REC_NV];
        int32_t *J = in_lds ? lds + 2 * np + lds[2 * p] : A.scratch + 2 * (o + ALD_REC_HDR);
        bool inside = true;
        for(int i = 0; i < n; i++) if(pv[i] >= (uint32_t)G.V) inside = false;
        int nj = 0;
        if(inside) for(int i = 2; i + 1 < n; i++) if(G.lpos[pv[i]] != G.rpos[pv[i - 1]]) { J[2 * nj] = (int32_t)pv[i - 1]; J[2 * nj + 1] = (int32_t)pv[i]; nj++; }
        if(in_lds) lds[2 * p + 1] = nj; else A.scratch[2 * o] = nj;
    }
    wsync_mem();

    // ---- the rows
    bool bad = false;
    for(int pid = lane; pid < np; pid += ALD_WAVE) {
        const unsigned long long o = A.index[gf + pid];
        ALD_GLOBAL const uint32_t *pv = A.pool + o + ALD_REC_HDR; const int n = (int)A.pool[o + ALD_REC_NV];
        ald_trst_features F = {};
        int done = 0;
        bool inside = true;
        for(int i = 0; i < n; i++) if(pv[i] >= (uint32_t)G.V) inside = false;
        if(n < 3 || !inside) { bad = true; A.rows[r0 + pid] = F; A.complete[r0 + pid] = 0; continue; }       // assert(n >= 3)
        F.num_vertices = n - 2; F.num_edges = n - 3; F.gr_vertices = G.V; F.gr_edges = G.E; F.gr_reads = ft_ix(A.gr_reads, g); F.gr_subgraph = ft_ix(A.gr_subgraph, g);
        F.max_mid_exon_len = 0;
        int nj = 0; const int32_t *J = ft_junc(A, lds, in_lds, np, gf, pid, nj);
        if(nj > 0) {
            {   // junctions over the span between the first and the last spliced vertex
                int is = -1, it = -1;
                for(int i = 0; i < n; i++) { if((int)pv[i] == J[0] && is < 0) is = i; if((int)pv[i] == J[2 * nj - 1]) it = i; }
                F.junc_ratio = 1.0 * nj / (it - is);
            }
            for(int i = 1; i < nj; i++) { const int len = G.rpos[J[2 * i]] - G.lpos[J[2 * i - 1]]; if(len > F.max_mid_exon_len) F.max_mid_exon_len = len; }
            const int sv = (int)pv[1], ev = (int)pv[n - 2];
            F.start_loss1 = ft_dx(A.loss1, G.ov + sv); F.start_loss2 = ft_dx(A.loss2, G.ov + sv); F.start_loss3 = ft_dx(A.loss3, G.ov + sv);
            F.end_loss1 = ft_dx(A.loss1, G.ov + ev); F.end_loss2 = ft_dx(A.loss2, G.ov + ev); F.end_loss3 = ft_dx(A.loss3, G.ov + ev);
            F.start_merged_loss = ft_dx(A.merged_loss, G.ov + sv); F.end_merged_loss = ft_dx(A.merged_loss, G.ov + ev);
            // unique_junc: junctions of this path that no other path of the graph has (lists ascend in their first vertex)
            for(int j = 0; j < nj; j++) {
                const int a = J[2 * j], c = J[2 * j + 1]; bool shared = false;
                for(int q = 0; q < np && !shared; q++) {
                    if(q == pid) continue;
                    int nk = 0; const int32_t *K = ft_junc(A, lds, in_lds, np, gf, q, nk);
                    for(int k = 0; k < nk; k++) { if(K[2 * k] > a) break; if(K[2 * k] == a && K[2 * k + 1] == c) { shared = true; break; } }
                }
                if(!shared) F.uni_junc++;
            }
            // introns of OTHER paths inside one exon of this path: before the first junction, between two, behind the last
            for(int q = 0; q < np && nj >= 2; q++) {
                if(q == pid) continue;
                int nk = 0; const int32_t *K = ft_junc(A, lds, in_lds, np, gf, q, nk);
                if(nk == 0) continue;
                int mid = 0, head = 0, tail = 0;
                for(int i = 0; i < nj; i++) for(int k = 0; k < nk; k++) {
                    const int qa = K[2 * k], qb = K[2 * k + 1];
                    if(i == 0) { if(qa >= sv && qb <= J[0]) { head++; ft_ratio_of<RAW>(G, qa, qb, F.start_intron_ratio, bad); } }
                    else if(qb <= J[2 * i] && qa >= J[2 * i - 1]) { mid++; ft_ratio_of<RAW>(G, qa, qb, F.intron_ratio, bad); }
                    if(i == nj - 1) { if(qa >= J[2 * i + 1] && qb <= ev) { tail++; ft_ratio_of<RAW>(G, qa, qb, F.end_intron_ratio, bad); } }
                }
                if(F.introns < mid) F.introns = mid;
                if(F.start_introns < head) F.start_introns = head;
                if(F.end_introns < tail) F.end_introns = tail;
            }
            // along the path's own edges
            F.seq_min_wt = DBL_MAX; F.seq_min_cnt = INT_MAX; F.seq_min_abd = DBL_MAX; F.seq_min_ratio = 1.0;
            for(int i = 1; i < n; i++) {
                const int v1 = (int)pv[i - 1], v2 = (int)pv[i];
                const int e = ft_edge<RAW>(G, v1, v2);
                if(e < 0) { bad = true; continue; }
                const double w = G.ew[e], r = w / ft_dmax(ft_in_weights<RAW>(G, v2), ft_out_weights<RAW>(G, v1));
                const int cnt = G.ecount[e]; const double abd = G.eabd[e];
                F.seq_min_wt = ft_dmin(F.seq_min_wt, w); F.seq_min_cnt = ft_imin(F.seq_min_cnt, cnt); F.seq_min_abd = ft_dmin(F.seq_min_abd, abd); F.seq_min_ratio = ft_dmin(F.seq_min_ratio, r);
                F.seq_max_wt = ft_dmax(F.seq_max_wt, w); F.seq_max_cnt = ft_imax(F.seq_max_cnt, cnt); F.seq_max_abd = ft_dmax(F.seq_max_abd, abd); F.seq_max_ratio = ft_dmax(F.seq_max_ratio, r);
                if(i == 1) { F.unbridge_start_coming_count = ft_ix(A.coming_count, G.ov + v2); F.unbridge_start_coming_ratio = ft_dx(A.coming_ratio, G.ov + v2); F.start_cnt = cnt; F.start_weight = w; F.start_abd = abd; }
                else if(i == n - 2) { F.unbridge_end_leaving_count = ft_ix(A.leaving_count, G.ov + v2); F.unbridge_end_leaving_ratio = ft_dx(A.leaving_ratio, G.ov + v2); }
                else if(i == n - 1) { F.end_cnt = cnt; F.end_weight = w; F.end_abd = abd; }
            }
            done = 1;
        }
        A.rows[r0 + pid] = F; A.complete[r0 + pid] = done;
    }
    const bool any_bad = wballot(bad) != 0;
    if(lane == 0) A.graph_rc[g] = any_bad ? ALD_ST_INVARIANT + ALD_INV_OTHER : ALD_OK;
}

ALD_INL void features_graph(const FeatArgs &A, int g, int32_t *lds)
{
    if(A.in.g_rawdist && A.in.g_rawdist[g] >= 0) {
        if(A.g_ew) features_graph_t<true>(A, g, lds);                // (no overlay: the raw graphs are the host routine's)
        return;
    }
    features_graph_t<false>(A, g, lds);
}

} // namespace ald
