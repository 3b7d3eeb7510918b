// flat_rows_main.cc -- the flat transcript set's column view, row operations and merge order (aletsch_amd/csrc/tset_flat.h) on the
// smallest shapes that can go wrong, as a stand-alone program: tests/test_tset_flat_cpu.py builds it with ASan + UBSan and runs it.
// Exit status 0 and "flat rows ok" when every check holds.
#include "../aletsch_amd/csrc/tset_flat.h"
#include "../aletsch_amd/host/transcript_sink.hpp"
#include <cstdio>

using namespace ald;
using aletsch::sink_item; using aletsch::sink_transcript; using aletsch::transcript_sink;

static int failures = 0;
#define CHECK(c) do { if(!(c)) { failures++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while(0)

static sink_transcript tx(char strand, double cov, int64_t tid, std::initializer_list<int32_t> xs)
{
    sink_transcript t; t.strand = strand; t.coverage = cov; t.top.cov2 = cov; t.top.conf = cov / 2; t.top.abd = cov * 3; t.top.count1 = (int)tid % 7; t.count2 = 1; t.tid = tid;
    t.xs.assign(xs.begin(), xs.end());
    return t;
}
static ald_tset_flat flatten(const transcript_sink &s)
{
    const SinkRows R = sink_rows(&s, 1);
    ald_tset_flat F; flat_resize(F, (int64_t)R.item.size(), R.ne, R.ns);
    const FlatMut V = flat_mut(F);
    for(int64_t i = 0; i < V.n; i++) flat_put_item(V, i, R.hash[(size_t)i], *R.item[(size_t)i]);
    CHECK(F.exon_offset.back() == R.ne && F.sample_offset.back() == R.ns);
    return F;
}
static transcript_sink sink_of(const ald_tset_flat &F)          // what ald_tset_add_flat does with a flat set, into a fresh sink
{
    transcript_sink s; const FlatView v = flat_view(F);
    for(int64_t i = 0; i < v.n; ) {
        transcript_sink::bucket b; int64_t j = i;
        for(; j < v.n && v.hash[j] == v.hash[i]; j++) b.push_back(flat_get_item(v, j));
        s.add_bucket((size_t)v.hash[i], b); i = j;
    }
    return s;
}
static bool same(const ald_tset_flat &a, const ald_tset_flat &b) { bool eq = true; for_each_column([&](FlatKind, const auto &x, const auto &y) { eq = eq && x == y; }, a, b); return eq; }
static bool same_item(const sink_item &a, const sink_item &b)
{
    bool eq = a.count == b.count && a.trst.strand == b.trst.strand && a.trst.coverage == b.trst.coverage && a.trst.count2 == b.trst.count2 && a.trst.tid == b.trst.tid && a.trst.xs.size() == b.trst.xs.size()
              && a.trst.top.cov2 == b.trst.top.cov2 && a.trst.top.conf == b.trst.top.conf && a.trst.top.abd == b.trst.top.abd && a.trst.top.count1 == b.trst.top.count1 && a.samples.size() == b.samples.size();
    for(size_t k = 0; eq && k < a.trst.xs.size(); k++) eq = a.trst.xs[k] == b.trst.xs[k];
    for(size_t k = 0; eq && k < a.samples.size(); k++) {
        const auto &p = a.samples.v[k], &q = b.samples.v[k];
        eq = p.first == q.first && p.second.coverage == q.second.coverage && p.second.count2 == q.second.count2 && p.second.top.cov2 == q.second.top.cov2 && p.second.top.conf == q.second.top.conf
             && p.second.top.abd == q.second.top.abd && p.second.top.count1 == q.second.top.count1;
    }
    return eq;
}
// sink -> rows -> sink_item -> a fresh sink -> rows: the same columns and the same items; the set through its wire form, the exports'
// copy-out and a row-by-row copy: the same columns
static void round_trip(const transcript_sink &s, int64_t n, int64_t ne, int64_t ns)
{
    const ald_tset_flat F = flatten(s);
    const FlatView v = flat_view(F);
    CHECK(v.n == n && v.ne == ne && v.ns == ns);
    const transcript_sink s2 = sink_of(F);
    CHECK(same(F, flatten(s2)));
    const SinkRows a = sink_rows(&s, 1), b = sink_rows(&s2, 1);
    CHECK(a.item.size() == b.item.size() && a.hash == b.hash);
    for(size_t i = 0; i < a.item.size() && i < b.item.size(); i++) CHECK(same_item(*a.item[i], *b.item[i]));
    std::vector<uint64_t> wire; flat_pack(v, wire);
    FlatView w; CHECK(flat_unpack(wire.data(), (int64_t)wire.size(), w));
    CHECK(!flat_unpack(wire.data(), (int64_t)wire.size() - 1, w));
    CHECK(flat_unpack(wire.data(), (int64_t)wire.size(), w));
    ald_tset_flat G, R; flat_resize(G, n, ne, ns); flat_resize(R, n, ne, ns);
    if(ne && ns) { FlatMut m = flat_mut(G); CHECK(!flat_has_null(m)); m.sample_abd = nullptr; CHECK(flat_has_null(m)); }
    flat_copy(flat_mut(G), w);
    CHECK(same(F, G));
    for(int64_t i = 0; i < n; i++) flat_copy_row(flat_mut(R), i, w, i);
    CHECK(same(F, R));
}
static bool order_is(const std::vector<std::vector<uint64_t>> &src, std::initializer_list<std::pair<int32_t, int64_t>> want)
{
    std::vector<HashRun> runs; for(auto &x : src) runs.push_back(HashRun{x.data(), (int64_t)x.size()});
    return merge_order(runs) == std::vector<std::pair<int32_t, int64_t>>(want);
}

int main()
{
    { transcript_sink s; round_trip(s, 0, 0, 0); }                                                  // an empty set
    { transcript_sink s; transcript_sink::bucket b; sink_item z; z.trst = tx('+', 1.5, 11, {100, 200, 300, 400}); z.count = 2; b.push_back(z);      // one item without a sample
      s.add_bucket(z.trst.chain_key(), b); round_trip(s, 1, 2, 0); }
    { transcript_sink s; s.add(tx('.', 0.25, 5, {}), 1, 3); CHECK(s.mt.find(0) != s.mt.end()); round_trip(s, 1, 0, 1); }       // the item without an exon, bucket 0, alone: no exon column to write to
    { transcript_sink s;                                                                            // bucket 0 among others, one exon, nine exons (beyond the eight an item holds inline), shared samples
      s.add(tx('.', 0.25, 5, {}), 1, 3);
      s.add(tx('+', 2.0, 6, {1000, 1500}), 1, 0); s.add(tx('+', 3.0, 7, {1100, 1600}), 1, 2);        // overlap: one item, two samples
      s.add(tx('-', 4.0, 8, {10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120, 130, 140, 150, 160, 170, 180}), 1, 1);
      s.add(tx('-', 5.0, 9, {12, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120, 130, 140, 150, 160, 170, 190}), 2, 4);      // the same chain: merged, bounds widened
      s.add(tx('+', 6.0, 10, {10, 20, 30, 40}), 1, 1);
      round_trip(s, 4, 12, 6); }
    // merge order: a bucket in two sources (lower source first, each taken whole), two items of one bucket in one source, an empty source
    CHECK(order_is({{1, 5, 5, 9}, {2, 5, 7}}, {{0, 0}, {1, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {0, 3}}));
    CHECK(order_is({{4, 4, 8}, {}, {3, 4, 8, 8}}, {{2, 0}, {0, 0}, {0, 1}, {2, 1}, {0, 2}, {2, 2}, {2, 3}}));
    CHECK(order_is({{}, {}}, {}));
    CHECK(order_is({{}, {7}}, {{1, 0}}));
    if(failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("flat rows ok\n");
    return 0;
}
