// tset_flat.h -- the FLAT transcript set, the form in which a finished set leaves the library (ald_tset_export, ald_tset_flat_export,
// ald_tset_dev_export): 18 columns.  for_each_column names every column ONCE with its kind; whatever treats columns in bulk (sizing, the
// exports' null check and copy-out, the wire form of ald_comm_gather_sets, the device -> host fetch, a row copy) goes through it, so a new column
// is one more entry there plus its place in a row.  Plain host C++ (tests/flat_rows_main.cc runs it under ASan + UBSan).  Not installed, not ABI.
#pragma once
#include "host_pack.h"                      // rvec
#include "../host/transcript_sink.hpp"
#include <type_traits>
using ald::rvec;
// the reduced set of one batch, flat, in the reference's iteration order (ascending bucket hash, bucket order inside)
struct ald_tset_flat {      // (rvec: sized once, every element written by the parallel fill -- no zero pass over ~200 MB first)
    rvec<uint64_t> hash; rvec<int32_t> count, count1, count2; rvec<char> strand; rvec<double> coverage, cov2, conf, abd; rvec<int64_t> tid; std::vector<int64_t> exon_offset, sample_offset;
    rvec<int32_t> exon_lr, sample_sid, sample_count1; rvec<double> sample_cov2, sample_conf, sample_abd;
    double device_ms = 0, host_ms = 0; int64_t n_device_groups = 0, n_host_items = 0;
};

namespace ald {
enum FlatKind { PER_ITEM, PER_ITEM1, PER_EXON, PER_SAMPLE };      // elements of a column for n items, ne exon pairs, ns samples:
inline size_t flat_len(FlatKind k, int64_t n, int64_t ne, int64_t ns) { return (size_t)(k == PER_ITEM ? n : k == PER_ITEM1 ? n + 1 : k == PER_EXON ? 2 * ne : ns); }
// f(kind, column of the first set, column of the second, ...) for every column, in the order of the exports' arguments (which is also
// the wire order).  A set: anything with these members -- an ald_tset_flat (vectors), a FlatCols (pointers).
template<class F, class... S> void for_each_column(F f, S &&... s)
{
    f(PER_ITEM, s.hash...); f(PER_ITEM, s.count...); f(PER_ITEM, s.strand...); f(PER_ITEM, s.coverage...); f(PER_ITEM, s.cov2...); f(PER_ITEM, s.conf...); f(PER_ITEM, s.abd...);
    f(PER_ITEM, s.count1...); f(PER_ITEM, s.count2...); f(PER_ITEM, s.tid...); f(PER_ITEM1, s.exon_offset...); f(PER_EXON, s.exon_lr...);
    f(PER_ITEM1, s.sample_offset...); f(PER_SAMPLE, s.sample_sid...); f(PER_SAMPLE, s.sample_cov2...); f(PER_SAMPLE, s.sample_conf...); f(PER_SAMPLE, s.sample_abd...); f(PER_SAMPLE, s.sample_count1...);
}
// the columns as pointers (an aggregate: the 18 arguments of an export entry point in their order, then n, ne, ns)
template<bool Mut> struct FlatCols {
    template<class T> using P = typename std::conditional<Mut, T, const T>::type *;
    P<uint64_t> hash; P<int32_t> count; P<char> strand; P<double> coverage, cov2, conf, abd; P<int32_t> count1, count2; P<int64_t> tid, exon_offset; P<int32_t> exon_lr;
    P<int64_t> sample_offset; P<int32_t> sample_sid; P<double> sample_cov2, sample_conf, sample_abd; P<int32_t> sample_count1;
    int64_t n, ne, ns; size_t len(FlatKind k) const { return flat_len(k, n, ne, ns); }
};
typedef FlatCols<true> FlatMut; typedef FlatCols<false> FlatView;
template<class V, class Flat> V flat_cols_of(Flat &f)
{
    V v; for_each_column([](FlatKind, auto &p, auto &col) { p = col.data(); }, v, f);
    v.n = (int64_t)f.hash.size(); v.ne = (int64_t)f.exon_lr.size() / 2; v.ns = (int64_t)f.sample_sid.size(); return v;
}
inline FlatMut flat_mut(ald_tset_flat &f) { return flat_cols_of<FlatMut>(f); }
inline FlatView flat_view(const ald_tset_flat &f) { return flat_cols_of<FlatView>(f); }
// every column sized for (n, ne, ns).  What is there stays; new elements of the two offset columns are zero, the others unwritten
inline void flat_resize(ald_tset_flat &f, int64_t n, int64_t ne, int64_t ns) { for_each_column([&](FlatKind k, auto &col) { col.resize(flat_len(k, n, ne, ns)); }, f); }
template<bool Mut> bool flat_has_null(const FlatCols<Mut> &v) { bool bad = false; for_each_column([&](FlatKind, auto p) { bad |= !p; }, v); return bad; }
inline void flat_copy(const FlatMut &dst, const FlatView &src) { for_each_column([&](FlatKind k, auto d, auto s) { if(src.len(k)) memcpy(d, s, sizeof(*s) * src.len(k)); }, dst, src); }
// a set as ONE run of 8-byte words: n, ne, ns, then every column, each padded to a multiple of 8 bytes
inline void flat_pack(const FlatView &v, std::vector<uint64_t> &buf)
{
    buf.assign({(uint64_t)v.n, (uint64_t)v.ne, (uint64_t)v.ns});
    for_each_column([&](FlatKind k, auto p) { const size_t bytes = v.len(k) * sizeof(*p), at = buf.size(); buf.resize(at + (bytes + 7) / 8, 0); if(bytes) memcpy(buf.data() + at, p, bytes); }, v);
}
// ... and a view into such a run; false unless the counts, the run's length and the last offsets agree
inline bool flat_unpack(const uint64_t *p, int64_t words, FlatView &v)
{
    if(words < 3) return false;
    v.n = (int64_t)p[0]; v.ne = (int64_t)p[1]; v.ns = (int64_t)p[2]; size_t at = 3;
    if(v.n < 0 || v.ne < 0 || v.ns < 0 || v.n > words || v.ne > words || v.ns > words) return false;
    for_each_column([&](FlatKind k, auto &col) { if(at <= (size_t)words) col = (typename std::remove_reference<decltype(col)>::type)(p + at); at += (v.len(k) * sizeof(*col) + 7) / 8; }, v);
    return at == (size_t)words && v.exon_offset[v.n] == v.ne && v.sample_offset[v.n] == v.ns;
}
// ---- rows.  A row that is written begins where the row before it ended -- exon_offset[i] / sample_offset[i], zero for row 0 or set ahead
// of a fill that does not go in order -- and leaves its own end in [i + 1].
// a host sink item, filed under `hash`, into row i
inline void flat_put_item(const FlatMut &v, int64_t i, uint64_t hash, const aletsch::sink_item &z)
{
    const aletsch::sink_transcript &r = z.trst; const int64_t e = v.exon_offset[i]; int64_t s = v.sample_offset[i];
    v.hash[i] = hash; v.count[i] = z.count; v.strand[i] = r.strand; v.coverage[i] = r.coverage; v.cov2[i] = r.top.cov2; v.conf[i] = r.top.conf; v.abd[i] = r.top.abd; v.count1[i] = r.top.count1; v.count2[i] = r.count2; v.tid[i] = r.tid;
    if(!r.xs.empty()) memcpy(v.exon_lr + 2 * e, r.xs.data(), 4 * r.xs.size());      // (bucket 0 holds the item without an exon)
    for(auto &q : z.samples) { v.sample_sid[s] = q.first; v.sample_cov2[s] = q.second.top.cov2; v.sample_conf[s] = q.second.top.conf; v.sample_abd[s] = q.second.top.abd; v.sample_count1[s] = q.second.top.count1; s++; }
    v.exon_offset[i + 1] = e + (int64_t)r.n_exons(); v.sample_offset[i + 1] = s;
}
// ... and back: the sink item row k holds (every per-sample copy mirrors the item's coverage and count2, sink_item::settle)
inline aletsch::sink_item flat_get_item(const FlatView &v, int64_t k)
{
    aletsch::sink_item z; aletsch::sink_transcript &r = z.trst;
    r.strand = v.strand[k]; r.coverage = v.coverage[k]; r.top.cov2 = v.cov2[k]; r.top.conf = v.conf[k]; r.top.abd = v.abd[k]; r.top.count1 = v.count1[k]; r.count2 = v.count2[k]; r.tid = v.tid[k];
    r.xs.assign(v.exon_lr + 2 * v.exon_offset[k], v.exon_lr + 2 * v.exon_offset[k + 1]); z.count = v.count[k];
    for(int64_t s = v.sample_offset[k]; s < v.sample_offset[k + 1]; s++) {
        aletsch::sink_sample x; x.coverage = r.coverage; x.top.cov2 = v.sample_cov2[s]; x.top.conf = v.sample_conf[s]; x.top.abd = v.sample_abd[s]; x.top.count1 = v.sample_count1[s]; x.count2 = r.count2;
        bool fresh; z.samples.slot(v.sample_sid[s], x, fresh);
    }
    return z;
}
// row i of `src` into row k of `dst` (the caller has checked src's offsets where they come from outside)
inline void flat_copy_row(const FlatMut &dst, int64_t k, const FlatView &src, int64_t i)
{
    const int64_t e = dst.exon_offset[k], s = dst.sample_offset[k], e0 = src.exon_offset[i], ne = src.exon_offset[i + 1] - e0, s0 = src.sample_offset[i], ns = src.sample_offset[i + 1] - s0;
    for_each_column([&](FlatKind kind, auto d, auto c) {
        if(kind == PER_ITEM) d[k] = c[i];
        else if(kind == PER_EXON) { if(ne) memcpy(d + 2 * e, c + 2 * e0, sizeof(*c) * 2 * (size_t)ne); }
        else if(kind == PER_SAMPLE) for(int64_t q = 0; q < ns; q++) d[s + q] = c[s0 + q];
    }, dst, src);
    dst.exon_offset[k + 1] = e + ne; dst.sample_offset[k + 1] = s + ns;
}
// the items of sinks with disjoint key sets in the reference's iteration order (ascending key, bucket order inside) + their exon / sample totals
struct SinkRows { std::vector<uint64_t> hash; std::vector<const aletsch::sink_item*> item; int64_t ne = 0, ns = 0; };
inline SinkRows sink_rows(const aletsch::transcript_sink *sinks, size_t n_sinks)
{
    std::vector<std::pair<size_t, const aletsch::transcript_sink::bucket*>> b; SinkRows R;
    for(size_t k = 0; k < n_sinks; k++) for(auto &x : sinks[k].mt) b.emplace_back(x.first, &x.second);
    std::sort(b.begin(), b.end());
    for(auto &x : b) for(auto &z : *x.second) { R.hash.push_back((uint64_t)x.first); R.item.push_back(&z); R.ne += (int64_t)z.trst.n_exons(); R.ns += (int64_t)z.samples.size(); }
    return R;
}
// The order in which K sources of ascending hashes merge, as (source, index): the smallest bucket at a head next, taken whole; a bucket
// that several sources hold comes from the lower source first (fewer exons sort first, transcript.cc:271: the host part goes in front).
struct HashRun { const uint64_t *hash; int64_t n; };
inline std::vector<std::pair<int32_t, int64_t>> merge_order(const std::vector<HashRun> &src)
{
    std::vector<std::pair<int32_t, int64_t>> out; size_t N = 0; for(auto &x : src) N += (size_t)x.n;
    out.reserve(N);
    for(std::vector<int64_t> cur(src.size(), 0); out.size() < N; ) {
        int best = -1;
        for(int r = 0; r < (int)src.size(); r++) if(cur[(size_t)r] < src[(size_t)r].n && (best < 0 || src[(size_t)r].hash[cur[(size_t)r]] < src[(size_t)best].hash[cur[(size_t)best]])) best = r;
        const HashRun &x = src[(size_t)best]; int64_t &i = cur[(size_t)best]; const uint64_t h = x.hash[i];
        while(i < x.n && x.hash[i] == h) out.emplace_back(best, i++);
    }
    return out;
}
} // namespace ald
