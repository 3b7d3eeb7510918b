// record_layout_test.cc -- aletsch_amd/csrc/record_layout.h against the two formats as include/aletsch_decomp.h describes them in prose:
//   path record    [graph, path index, #vertices, length, count, strand | attempt<<8, weight f64, abd f64, conf f64, reads f64,
//                   #exon words, 0, vertices..., exon words (l, r)*..., pad to even]
//   stream record  [graph, path index, sid, strand, count1, n_exons, weight f64, conf f64, abd f64, (l, r) * n_exons]
// Every expected word below is written out by hand from those two lines; nothing here uses the ALD_REC_* / ALD_TS_* names to say what
// a word should be.  Host code only; the CPU tier builds it plain and with ASan + UBSan (tests/test_record_layout_cpu.py).
#include "../../aletsch_amd/csrc/record_layout.h"
#include <cstdio>
#include <cstdlib>

using namespace ald;

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while(0)

static double from_bits(uint32_t lo, uint32_t hi) { const uint64_t b = ((uint64_t)hi << 32) | lo; double d; memcpy(&d, &b, 8); return d; }

int main()
{
    // four different doubles whose low AND high words are pairwise distinct (little endian: the low word comes first)
    const uint32_t W_LO = 0x11111111u, W_HI = 0x3FF80000u;      // weight  ~1.5
    const uint32_t A_LO = 0x22222222u, A_HI = 0x40020000u;      // abd     ~2.25
    const uint32_t C_LO = 0x33333333u, C_HI = 0x3FE40000u;      // conf    ~0.625
    const uint32_t R_LO = 0x44444444u, R_HI = 0x40238000u;      // reads   ~9.75
    const double weight = from_bits(W_LO, W_HI), abd = from_bits(A_LO, A_HI), conf = from_bits(C_LO, C_HI), reads = from_bits(R_LO, R_HI);

    // the path record, filled by literal index: graph 5, path 9, 3 vertices, length 11, count 7, strand '-', attempt 3, 4 exon words
    uint32_t rec[24];
    for(int i = 0; i < 24; i++) rec[i] = 0xDEAD0000u + (uint32_t)i;
    rec[0] = 5; rec[1] = 9; rec[2] = 3; rec[3] = 11; rec[4] = 7; rec[5] = (uint32_t)'-' | (3u << 8);
    memcpy(rec + 6, &weight, 8); memcpy(rec + 8, &abd, 8); memcpy(rec + 10, &conf, 8); memcpy(rec + 12, &reads, 8);
    rec[14] = 4; rec[15] = 0;
    rec[16] = 0; rec[17] = 4; rec[18] = 8;                       // vertices
    rec[19] = 100; rec[20] = 200; rec[21] = 300; rec[22] = 400;  // exons
    rec[23] = 0;                                                 // pad: 16 + 3 + 4 = 23 words -> 24

    // ---- accessors of the path record
    CHECK(rec_strand(rec) == (uint32_t)'-' && rec_attempt(rec) == 3);
    CHECK(rec_f64(rec, 6) == weight && rec_f64(rec, 8) == abd && rec_f64(rec, 10) == conf && rec_f64(rec, 12) == reads);
    CHECK(rec_f64(rec, ALD_REC_WEIGHT) == weight && rec_f64(rec, ALD_REC_ABD) == abd && rec_f64(rec, ALD_REC_CONF) == conf && rec_f64(rec, ALD_REC_READS) == reads);
    CHECK(rec_f64_slot(ALD_REC_WEIGHT) == 0 && rec_f64_slot(ALD_REC_ABD) == 1 && rec_f64_slot(ALD_REC_CONF) == 2 && rec_f64_slot(ALD_REC_READS) == 3);
    CHECK(rec_vertices(rec) == rec + 16 && rec_vertices(rec)[1] == 4);
    CHECK(rec_exons(rec) == (const int32_t*)(rec + 16 + 3) && rec_exons(rec)[0] == 100 && rec_exons(rec)[3] == 400);
    CHECK(rec_words(2, 0) == 18 && rec_words(2, 2) == 20 && rec_words(3, 2) == 22 && rec_words(3, 4) == 24);
    CHECK(rec_words(rec[2], rec[14]) == 24);
    CHECK(REC_HDR_WORDS == 16 && REC_NEXW == 14);               // the older names of the header length and the exon-word count stay

    // ---- path record -> stream header: conf BEFORE abd
    int32_t sid[6] = {60, 61, 62, 63, 64, 41};                   // graph 5 -> sample 41
    const uint32_t want_ts[12]      = {5, 9, 41,          (uint32_t)'-', 7, 2, W_LO, W_HI, C_LO, C_HI, A_LO, A_HI};
    const uint32_t want_ts_nosid[12] = {5, 9, 0xFFFFFFFFu, (uint32_t)'-', 7, 2, W_LO, W_HI, C_LO, C_HI, A_LO, A_HI};
    uint32_t ts[12 + 4];
    for(int l = 0; l < 12; l++) {
        ts[l] = ts_header_word(rec, l, sid);
        CHECK(ts[l] == want_ts[l]);
        CHECK(ts_header_word(rec, l, nullptr) == want_ts_nosid[l]);
    }
    memcpy(ts + 12, rec_exons(rec), 16);

    // ---- accessors of the stream record
    CHECK(ts_f64(ts, 6) == weight && ts_f64(ts, 8) == conf && ts_f64(ts, 10) == abd);
    CHECK(ts_f64(ts, ALD_TS_WEIGHT) == weight && ts_f64(ts, ALD_TS_CONF) == conf && ts_f64(ts, ALD_TS_ABD) == abd);
    CHECK(ts_exons(ts) == (const int32_t*)(ts + 12) && ts_exons(ts)[2] == 300);
    CHECK(ts_nexw(ts) == 4 && ts_words(ts) == 16);
    { uint32_t h[12] = {0}; h[5] = 0; CHECK(ts_nexw(h) == 0 && ts_words(h) == 12); h[5] = 1; CHECK(ts_nexw(h) == 2 && ts_words(h) == 14); h[5] = 2; CHECK(ts_words(h) == 16);
      h[5] = 0x7FFFFFFFu; CHECK(ts_words(h) == 12 + 2 * (int64_t)0x7FFFFFFF); }      // 64-bit: no wrap at the largest exon count

    // ---- stream record -> scratch record header: abd BEFORE conf, two vertices, zeros for length / attempt / reads / word 15
    const int32_t gid1 = 3;                                      // 1-based group 3 -> graph word 2
    const uint32_t want_rec[16] = {2, 9, 2, 0, 7, (uint32_t)'-', W_LO, W_HI, A_LO, A_HI, C_LO, C_HI, 0, 0, 4, 0};
    uint32_t back[16];
    for(int l = 0; l < 16; l++) { back[l] = rec_header_word_of_ts(ts, l, &gid1); CHECK(back[l] == want_rec[l]); }
    { uint32_t t2[12]; memcpy(t2, ts, 48); t2[3] = 0xABCD0000u | (uint32_t)'+'; CHECK(rec_header_word_of_ts(t2, 5, &gid1) == (uint32_t)'+'); }   // only the strand byte is taken

    // ---- rec -> ts -> rec keeps graph, path, count, strand, weight, abd, conf
    const int32_t same_graph = 5 + 1;
    CHECK(rec_header_word_of_ts(ts, 0, &same_graph) == rec[0]);
    CHECK(back[1] == rec[1] && back[4] == rec[4] && rec_strand(back) == rec_strand(rec));
    CHECK(rec_f64(back, 6) == weight && rec_f64(back, 8) == abd && rec_f64(back, 10) == conf);
    CHECK(back[14] == rec[14] && rec_words(back[2], back[14]) == 22);

    if(fails) { std::printf("record layout: %d checks failed\n", fails); return 1; }
    std::printf("record layout ok\n");
    return 0;
}
