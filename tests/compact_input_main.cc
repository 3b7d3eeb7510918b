// compact_input_main.cc -- CPU tier of the compact-input tests: the host side of the mode (HostBatch in host_pack.h), stand-alone, built with
// g++ -fsanitize=address,undefined by tests/test_compact_input_cpu.py.  For every case of compact_input_cases.h, staged packed and
// graph by graph:
//   * layout() of a compact batch reserves every section where an eager batch has it and marks exactly the expected ones derived;
//   * after ensure_in_csr() every array of the compact batch equals the eager batch's, byte for byte;
// then: a defective graph in the middle of an add_packed call rolls a batch back to what it was (flags and per-graph sample ids
// included), and clear() + reuse gives what a fresh batch gives.  Prints one line per check that fails; exit status 1 if any did.
#include "compact_input_cases.h"
#include <cstdio>

using namespace cic;
typedef HostBatch::Section Sec;
static int failures = 0;
#define FAIL(...) do { failures++; printf("FAIL "); printf(__VA_ARGS__); printf("\n"); } while(0)

static uint64_t full_layout(HostBatch &B, Sec *sec)          // (the eager view of a compact batch: every section has its source)
{
    const bool was = B.compact;
    B.ensure_in_csr(); B.compact = false; const uint64_t bytes = B.layout(sec); B.compact = was;
    return bytes;
}
// every section of C against E (either may be compact: its in-CSR is ensured first): same place, same size, same bytes; same flags
static void same_arrays(const std::string &what, HostBatch &C, HostBatch &E)
{
    Sec sc[HostBatch::S_COUNT], se[HostBatch::S_COUNT];
    const uint64_t bc = full_layout(C, sc), be = full_layout(E, se);
    if(bc != be) FAIL("%s: buffer of %llu bytes, eager %llu", what.c_str(), (unsigned long long)bc, (unsigned long long)be);
    for(int i = 0; i < HostBatch::S_COUNT; i++) {
        if(sc[i].bytes != se[i].bytes || sc[i].off != se[i].off) { FAIL("%s: section %s at %llu + %llu, eager %llu + %llu", what.c_str(), section_name(i), (unsigned long long)sc[i].off, (unsigned long long)sc[i].bytes, (unsigned long long)se[i].off, (unsigned long long)se[i].bytes); continue; }
        if(sc[i].bytes && memcmp(sc[i].src, se[i].src, sc[i].bytes) != 0) FAIL("%s: section %s differs from the eager batch", what.c_str(), section_name(i));
    }
    if(C.def_eabd != E.def_eabd || C.def_ecount != E.def_ecount || C.def_vtype != E.def_vtype || C.def_estrand != E.def_estrand) FAIL("%s: default flags differ from the eager batch", what.c_str());
    if(!E.compact && (!E.uni_samples || !E.g_sid.empty())) FAIL("%s: an eager batch tested its sample lists", what.c_str());      // work the full upload never did
    if(C.compact && (int)C.g_sid.size() != C.n()) FAIL("%s: %d per-graph sample ids for %d graphs", what.c_str(), (int)C.g_sid.size(), C.n());
    if(C.compact != E.compact) return;
    if(C.uni_samples != E.uni_samples) FAIL("%s: uni_samples differs from the control batch", what.c_str());
    if(C.g_sid.size() != E.g_sid.size() || (C.g_sid.size() && memcmp(C.g_sid.data(), E.g_sid.data(), 4 * C.g_sid.size()) != 0)) FAIL("%s: per-graph sample ids differ from the eager batch", what.c_str());
    if(C.compact && C.uni_samples) for(int g = 0; g < C.n(); g++) if(C.g_ne[g] > 0 && C.g_sid[(size_t)g] != C.sample_id[(size_t)C.off_s[g]]) FAIL("%s: g_sid[%d]", what.c_str(), g);
}
// the compact layout: every section where the eager layout has it, the expected ones derived and without a source
static void check_layout(const std::string &what, const HostBatch &C, const HostBatch &E, unsigned expect)
{
    Sec sc[HostBatch::S_COUNT], se[HostBatch::S_COUNT];
    const uint64_t bc = C.layout(sc), be = E.layout(se);
    if(bc != be) FAIL("%s: compact buffer of %llu bytes, eager %llu", what.c_str(), (unsigned long long)bc, (unsigned long long)be);
    const unsigned got = derive_mask(sc);
    if(got != expect) FAIL("%s: derived mask %u, expected %u", what.c_str(), got, expect);
    for(int i = 0; i < HostBatch::S_COUNT; i++) {
        if(sc[i].bytes != se[i].bytes || sc[i].off != se[i].off) FAIL("%s: compact section %s at %llu + %llu, eager %llu + %llu", what.c_str(), section_name(i), (unsigned long long)sc[i].off, (unsigned long long)sc[i].bytes, (unsigned long long)se[i].off, (unsigned long long)se[i].bytes);
        bool want = false;
        switch(i) {
            case HostBatch::S_INOFF: case HostBatch::S_INEDGE: want = expect & ALD_DERIVE_INCSR; break;
            case HostBatch::S_ESOFF: case HostBatch::S_SID: case HostBatch::S_SABD: want = expect & ALD_DERIVE_SAMPLES; break;
            case HostBatch::S_EABD: want = expect & ALD_DERIVE_EABD; break;
            case HostBatch::S_ECOUNT: want = expect & ALD_DERIVE_ECOUNT; break;
            case HostBatch::S_VTYPE: want = expect & ALD_DERIVE_VTYPE; break;
            case HostBatch::S_ESTRAND: want = expect & ALD_DERIVE_ESTRAND; break;
            default: break;
        }
        if(sc[i].derived != want) FAIL("%s: section %s derived = %d, expected %d", what.c_str(), section_name(i), (int)sc[i].derived, (int)want);
        if(sc[i].derived && sc[i].src) FAIL("%s: derived section %s has a source", what.c_str(), section_name(i));
        if(se[i].derived) FAIL("%s: eager section %s marked derived", what.c_str(), section_name(i));
    }
}

int main()
{
    const std::vector<Case> all = cases();
    for(const Case &c : all) for(int packed = 0; packed < 2; packed++) {
        const std::string what = c.name + (packed ? " (packed)" : " (single)");
        HostBatch E, C; C.compact = true;
        const int re = stage(E, c, packed != 0), rc = stage(C, c, packed != 0);
        if(re != ALD_OK || rc != ALD_OK) { FAIL("%s: staging failed: %d %s / %d %s", what.c_str(), re, E.err.c_str(), rc, C.err.c_str()); continue; }
        if(!C.in_offset.empty() || !C.in_edge.empty()) FAIL("%s: the compact batch built an in-CSR at add", what.c_str());
        check_layout(what, C, E, c.expect);
        same_arrays(what, C, E);
        check_layout(what + " after ensure_in_csr", C, E, c.expect);                // a host reader's in-CSR does not make the section travel
    }
    // ---- a defective graph in the middle of an add_packed call: the batch goes back to what it was ----
    for(int compact = 0; compact < 2; compact++) {
        const std::string what = compact ? "rollback (compact)" : "rollback (eager)";
        HostBatch B, K; B.compact = K.compact = compact != 0;                       // K: the control, which never sees the bad call
        const std::vector<G> first = uniform_batch();
        std::vector<G> bad = {with_abd_count(with_type_strand(dag(8, 12, 3, 1))), with_abd_count(with_type_strand(chain(5))), with_abd_count(with_type_strand(dag(7, 9, 4, 2)))};
        bad[0].sid[3] = 7;                                   // would end the uniform sample lists ...
        bad[1].tgt[2] = 1;                                   // ... but this edge goes backwards: the call is refused
        if(stage_packed(B, first) != ALD_OK || stage_packed(K, first) != ALD_OK) { FAIL("%s: staging failed", what.c_str()); continue; }
        if(compact) B.ensure_in_csr();                       // a host reader came by: what it built of the graphs that stay is kept
        if(stage_packed(B, bad) == ALD_OK) FAIL("%s: the defective call was accepted", what.c_str());
        if(B.n() != K.n()) FAIL("%s: %d graphs left, expected %d", what.c_str(), B.n(), K.n());
        same_arrays(what, B, K);
        if(!B.uni_samples || !B.def_eabd || !B.def_vtype) FAIL("%s: a refused call left its marks on the flags", what.c_str());
        const std::vector<G> more = {chain(1030, 4, 3), in_fan(64, 1)};
        if(stage_packed(B, more) != ALD_OK || stage_packed(K, more) != ALD_OK) { FAIL("%s: staging after the rollback failed", what.c_str()); continue; }
        same_arrays(what + ", then more graphs", B, K);
        if(stage_single(B, bad[1]) == ALD_OK) FAIL("%s: the defective graph was accepted", what.c_str());
        same_arrays(what + ", then a refused add_graph", B, K);
    }
    // ---- clear and reuse ----
    {
        HostBatch C; C.compact = true;
        for(size_t i = 0; i + 1 < all.size(); i += 5) {
            const Case &a = all[i], &b = all[i + 1];
            C.clear(); if(stage(C, a, true) != ALD_OK) FAIL("reuse: staging %s failed", a.name.c_str());
            if(i % 2) C.ensure_in_csr();
            C.clear();
            if(!C.compact || !C.uni_samples || !C.def_eabd || !C.def_ecount || !C.def_vtype || !C.def_estrand || !C.g_sid.empty() || C.in_built != 0) FAIL("reuse: clear() after %s left state behind", a.name.c_str());
            HostBatch E;
            if(stage(C, b, false) != ALD_OK || stage(E, b, false) != ALD_OK) { FAIL("reuse: staging %s failed", b.name.c_str()); continue; }
            check_layout("reuse " + b.name, C, E, b.expect);
            same_arrays("reuse " + b.name, C, E);
        }
    }
    printf("%d cases, %d failures\n", (int)all.size(), failures);
    return failures ? 1 : 0;
}
