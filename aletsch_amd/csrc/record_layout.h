// record_layout.h -- the words of a PATH RECORD (what the decomposition kernel writes into the pool) and of a TRANSCRIPT-STREAM RECORD
// (ald_batch_transcript_stream), read and written through one set of names.  The word indices are ABI and live in
// include/aletsch_decomp.h (ALD_REC_*, ALD_TS_*); this header adds the accessors and the two translations between the formats.
// Compiles as host C++, as HIP device code and in the single-lane emulation (-DALD_EMU).  Not installed.
//
//   path record    [graph, path, #vertices, length, count, strand | attempt << 8, weight, ABD, CONF, reads (f64 each), #exon words, 0]
//                  [ALD_REC_HDR .. + #vertices) vertices, then the exon words (l, r)* of the transcript the path becomes -- touching
//                  vertex intervals joined, empty ones dropped (essential.cc:719-748) --, padded to an even word count
//   stream record  [graph, path, sid, strand, count1, n_exons, weight, CONF, ABD (f64 each)], then 2 * n_exons exon words
//
// The two formats hold conf and abd in OPPOSITE order; ts_header_word / rec_header_word_of_ts are the only places that swap them.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/aletsch_decomp.h"

#if defined(__HIP__)
  #define ALD_HD __host__ __device__
#else
  #define ALD_HD
#endif

namespace ald {

enum { REC_HDR_WORDS = ALD_REC_HDR, REC_NEXW = ALD_REC_NEXW };      // the names these two words had before the enums: kept for code outside the library that was built against them

// ---- path record
ALD_HD static inline unsigned long long rec_words(unsigned nv, unsigned nexw) { unsigned long long w = (unsigned long long)ALD_REC_HDR + nv + nexw; return w + (w & 1); }
ALD_HD static inline const uint32_t *rec_vertices(const uint32_t *r) { return r + ALD_REC_HDR; }
ALD_HD static inline const int32_t *rec_exons(const uint32_t *r) { return (const int32_t*)(r + ALD_REC_HDR + r[ALD_REC_NV]); }
ALD_HD static inline uint32_t rec_strand(const uint32_t *r) { return r[ALD_REC_STRAND] & 0xFF; }
ALD_HD static inline uint32_t rec_attempt(const uint32_t *r) { return (r[ALD_REC_STRAND] >> 8) & 0xFF; }
ALD_HD constexpr int rec_f64_slot(int word) { return (word - ALD_REC_WEIGHT) / 2; }     // the field's place in a double view of the record that begins at ALD_REC_WEIGHT (the kernel's stores)
// (tx_build, tx_fold and tx_sfold keep their memcpy into a declared double, with the named words: through rec_f64 the compiler emits
// different -- shorter -- loads for them, and a change of names is to leave every kernel as it was)
ALD_HD static inline double rec_f64(const uint32_t *r, int word) { double v; memcpy(&v, r + word, 8); return v; }
// the id of the transcript a path becomes; label: the graph id that goes into it (the graph's index, or what the caller numbers it)
ALD_HD static inline int64_t transcript_tid(int64_t tid_base, int64_t label, int64_t path) { return tid_base + ((label << 20) | path); }

// ---- transcript-stream record.  ts_words reads the header only: the caller checks that header and record lie inside its stream
ALD_HD static inline double ts_f64(const uint32_t *w, int word) { double v; memcpy(&v, w + word, 8); return v; }
ALD_HD static inline const int32_t *ts_exons(const uint32_t *w) { return (const int32_t*)(w + ALD_TS_HDR); }
ALD_HD static inline int64_t ts_nexw(const uint32_t *w) { return 2 * (int64_t)w[ALD_TS_NEXONS]; }
ALD_HD static inline int64_t ts_words(const uint32_t *w) { return (int64_t)ALD_TS_HDR + ts_nexw(w); }

// ---- the two translations, word by word: lane l of a kernel and step l of a host loop run the same code
// Each reads what only one word needs (the sample id, the group id) inside that word's case: in a kernel only the lane that writes the
// word loads it.
// header word l (0 .. ALD_TS_HDR - 1) of the stream record a path record becomes; sid: sample id per graph, or null (-1)
ALD_HD static inline uint32_t ts_header_word(const uint32_t *rec, int l, const int32_t *sid)
{
    const int g = (int)rec[ALD_REC_GRAPH];
    switch(l) {
    case ALD_TS_GRAPH:      return (uint32_t)g;
    case ALD_TS_PATH:       return rec[ALD_REC_PATH];
    case ALD_TS_SID:        return (uint32_t)(sid ? sid[g] : -1);
    case ALD_TS_STRAND:     return rec_strand(rec);
    case ALD_TS_COUNT1:     return rec[ALD_REC_COUNT];
    case ALD_TS_NEXONS:     return (uint32_t)((int)rec[ALD_REC_NEXW] / 2);
    case ALD_TS_WEIGHT:     return rec[ALD_REC_WEIGHT];
    case ALD_TS_WEIGHT + 1: return rec[ALD_REC_WEIGHT + 1];
    case ALD_TS_CONF:       return rec[ALD_REC_CONF];
    case ALD_TS_CONF + 1:   return rec[ALD_REC_CONF + 1];
    case ALD_TS_ABD:        return rec[ALD_REC_ABD];
    default:                return rec[ALD_REC_ABD + 1];
    }
}
// header word l (0 .. ALD_REC_HDR - 1) of the scratch record a stream record becomes: two (zero) vertices, no length, no reads, no
// attempt; gid1: where the 1-based group the front end files the record under lies (the stream index counts groups from 1)
ALD_HD static inline uint32_t rec_header_word_of_ts(const uint32_t *ts, int l, const int32_t *gid1)
{
    switch(l) {
    case ALD_REC_GRAPH:      return (uint32_t)(*gid1 - 1);
    case ALD_REC_PATH:       return ts[ALD_TS_PATH];
    case ALD_REC_NV:         return 2;
    case ALD_REC_COUNT:      return ts[ALD_TS_COUNT1];
    case ALD_REC_STRAND:     return ts[ALD_TS_STRAND] & 0xFF;
    case ALD_REC_WEIGHT:     return ts[ALD_TS_WEIGHT];
    case ALD_REC_WEIGHT + 1: return ts[ALD_TS_WEIGHT + 1];
    case ALD_REC_ABD:        return ts[ALD_TS_ABD];
    case ALD_REC_ABD + 1:    return ts[ALD_TS_ABD + 1];
    case ALD_REC_CONF:       return ts[ALD_TS_CONF];
    case ALD_REC_CONF + 1:   return ts[ALD_TS_CONF + 1];
    case ALD_REC_NEXW:       return (uint32_t)(2 * (int)ts[ALD_TS_NEXONS]);
    default:                 return 0;
    }
}

} // namespace ald
