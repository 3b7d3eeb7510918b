// stub_batch_abi.cc -- TEST-ONLY CPU stand-in for the batch entry points of the C ABI, so that the threaded host code above them --
// aletsch::gpu_assembly_queue (aletsch_amd/host/gpu_dispatch.hpp) and the result sink (aletsch_amd/csrc/ald_sink.cpp, linked AS IT IS) --
// runs in a program without a GPU, under ThreadSanitizer (tests/test_host_threads_cpu.py).
//
//   staging   the product's own HostBatch (host_pack.h), inside the product's own ald_batch (ald_internal.h; its device members stay unused)
//   run       the engine's single-lane emulation: emu_run_batch of tests/kernel_emu/emu_capi.cc, included below; the class objects
//             (tests/_build/emu_c*.o) are linked WITHOUT -fsanitize=thread -- single-threaded per call, and uninstrumented code can hide
//             a report, never invent one.  The emulation keeps diagnostic counters in globals, so one run at a time (g_emu)
//   download  the emulation's HostResults become the batch's: ald_tset_add_batch reads a batch filled as ald_batch_download fills it
//
// ald_tset_add_batch is the real one behind a counting / failing front: the test build compiles ald_sink.cpp with
// -Dald_tset_add_batch=ald_real_tset_add_batch.  Knobs: stub_control.h.
#ifndef ALD_EMU
#error "emulation build only (-DALD_EMU)"
#endif
#include "../../aletsch_amd/csrc/ald_internal.h"
#include "../kernel_emu/emu_capi.cc"
#include "stub_control.h"
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

extern "C" int ald_real_tset_add_batch(ald_tset *t, const ald_batch *b, const int32_t *sid, int64_t tid_base, int32_t skip_single_exon);

namespace {

thread_local std::string g_err;
std::mutex g_emu;

enum { E_ADD, E_UPLOAD, E_RUN, E_DOWNLOAD, E_MERGE, E_COUNT };
const char *const k_entry[E_COUNT] = {"add_packed", "upload", "run", "download", "tset_add_batch"};
std::atomic<long> g_calls[E_COUNT];
std::atomic<long> g_fail_at[E_COUNT];          // 0: never
std::atomic<int> g_fail_code[E_COUNT];
std::atomic<unsigned> g_delay_seed; std::atomic<int> g_delay_ms;
std::atomic<int> g_sink_width_min, g_stage_width_max;

int entry_of(const char *name) { for(int e = 0; e < E_COUNT; e++) if(name && !strcmp(name, k_entry[e])) return e; return -1; }
// counts the call; true (and the last-error text) when it is the one to fail
bool injected(int e, int &code)
{
    const long k = ++g_calls[e];
    if(k != g_fail_at[e].load()) return false;
    code = g_fail_code[e].load(); g_err = std::string("injected failure: ") + k_entry[e] + " call " + std::to_string(k);
    return true;
}
void device_delay(int device, long call)
{
    const int ms = g_delay_ms.load(); if(ms <= 0) return;
    uint64_t x = (uint64_t)g_delay_seed.load() * 0x9E3779B97F4A7C15ull + (uint64_t)device * 0xBF58476D1CE4E5B9ull + (uint64_t)call * 0x94D049BB133111EBull;
    x ^= x >> 31; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 29;
    std::this_thread::sleep_for(std::chrono::microseconds((long)(x % ((uint64_t)ms * 1000 + 1))));
}
void note_max(std::atomic<int> &a, int v) { int o = a.load(); while(v > o && !a.compare_exchange_weak(o, v)) {} }
void note_min(std::atomic<int> &a, int v) { int o = a.load(); while((o == 0 || v < o) && !a.compare_exchange_weak(o, v)) {} }

struct stub_batch : ald_batch { ald_params abi_prm; emu_result *pending = nullptr; ~stub_batch() { if(pending) emu_result_free(pending); } };
stub_batch *S(ald_batch *b) { return static_cast<stub_batch*>(b); }

template<class F> int staged(ald_batch *b, F add)
{
    int code; if(injected(E_ADD, code)) return code;
    b->uploaded = b->ran = b->downloaded = b->finished = false;
    const long before = thread_probe().peak; thread_probe().peak = 0;
    const int rc = add();
    note_max(g_stage_width_max, (int)thread_probe().peak + 1); thread_probe().peak = std::max(before, thread_probe().peak);
    if(rc != ALD_OK) g_err = b->hb.err;
    return rc;
}

} // namespace

int ald_set_err(int code, const std::string &msg) { g_err = msg; return code; }

extern "C" {

void stub_reset(void)
{
    for(int e = 0; e < E_COUNT; e++) { g_calls[e] = 0; g_fail_at[e] = 0; g_fail_code[e] = 0; }
    g_delay_seed = 0; g_delay_ms = 0; g_sink_width_min = 0; g_stage_width_max = 0;
}
void stub_set_delay(unsigned seed, int max_ms) { g_delay_seed = seed; g_delay_ms = max_ms; }
void stub_inject(const char *entry, long kth, int code) { const int e = entry_of(entry); if(e >= 0) { g_fail_code[e] = code; g_fail_at[e] = kth; } }
long stub_calls(const char *entry) { const int e = entry_of(entry); return e < 0 ? -1 : g_calls[e].load(); }
int stub_sink_width_min(void) { return g_sink_width_min.load(); }
int stub_stage_width_max(void) { return g_stage_width_max.load(); }

const char *ald_last_error(void) { return g_err.c_str(); }

int ald_batch_create(const ald_params *p, int device, ald_batch **out)
{
    if(!out || !p) return ALD_ERR_INVALID;
    stub_batch *b = new stub_batch();
    b->device = device; b->abi_prm = *p; params_from_abi(p, b->prm);
    b->hb.compact = (p->reserved & ALD_PARAM_COMPACT_INPUT) != 0;
    *out = b;
    return ALD_OK;
}
int ald_batch_destroy(ald_batch *b) { delete S(b); return ALD_OK; }
int ald_batch_clear(ald_batch *b)
{
    if(!b) return ALD_ERR_INVALID;
    b->hb.clear(); b->res.clear(); b->uploaded = b->ran = b->downloaded = b->finished = false;
    if(S(b)->pending) { emu_result_free(S(b)->pending); S(b)->pending = nullptr; }
    return ALD_OK;
}
int ald_batch_num_graphs(const ald_batch *b) { return b ? b->hb.n() : 0; }

int ald_batch_add_packed(ald_batch *b, int32_t n, const int32_t *g_nv, const int32_t *g_ne, const int32_t *g_np,
                         const int32_t *vertex_offset, const int32_t *edge_target, const double *edge_weight, const uint8_t *edge_strand, const double *edge_abd,
                         const int32_t *edge_sample_offset, const int32_t *sample_id, const double *sample_abd,
                         const double *vertex_weight, const int32_t *vertex_lpos, const int32_t *vertex_rpos, const int32_t *vertex_type,
                         const int32_t *phasing_offset, const int32_t *phasing_vertex, const int32_t *phasing_count, const char *graph_strand, const int32_t *edge_count,
                         const int32_t *edge_creation_rank)
{
    if(!b || n < 0 || !g_nv || !g_ne) return ALD_ERR_INVALID;
    return staged(b, [&] { return b->hb.add_packed(n, g_nv, g_ne, g_np, vertex_offset, edge_target, edge_weight, edge_strand, edge_abd, edge_sample_offset, sample_id, sample_abd,
                                                   vertex_weight, vertex_lpos, vertex_rpos, vertex_type, phasing_offset, phasing_vertex, phasing_count, graph_strand, edge_count, edge_creation_rank); });
}
int ald_batch_add_packed_raw(ald_batch *b, int32_t n, const int32_t *g_nv, const int32_t *g_ne, const int32_t *g_np,
                             const int32_t *vertex_offset, const int32_t *edge_target, const double *edge_weight, const uint8_t *edge_strand, const double *edge_abd,
                             const int32_t *edge_sample_offset, const int32_t *sample_id, const double *sample_abd,
                             const double *vertex_weight, const int32_t *vertex_lpos, const int32_t *vertex_rpos, const int32_t *vertex_type,
                             const int32_t *phasing_offset, const int32_t *phasing_vertex, const int32_t *phasing_count, const char *graph_strand, const int32_t *edge_count,
                             const int32_t *edge_creation_rank,
                             const int32_t *raw_max_group_boundary_distance, const int32_t *g_nphase, const int32_t *phase_offset, const int32_t *phase_coord, const int32_t *phase_count)
{
    if(!b || n < 0 || !g_nv || !g_ne) return ALD_ERR_INVALID;
    return staged(b, [&] { return b->hb.add_packed_raw(n, g_nv, g_ne, g_np, vertex_offset, edge_target, edge_weight, edge_strand, edge_abd, edge_sample_offset, sample_id, sample_abd,
                                                       vertex_weight, vertex_lpos, vertex_rpos, vertex_type, phasing_offset, phasing_vertex, phasing_count, graph_strand, edge_count, edge_creation_rank,
                                                       raw_max_group_boundary_distance, g_nphase, phase_offset, phase_coord, phase_count); });
}

int ald_batch_upload(ald_batch *b)
{
    if(!b) return ALD_ERR_INVALID;
    int code; if(injected(E_UPLOAD, code)) return code;
    b->uploaded = true; b->ran = b->downloaded = b->finished = false;
    return ALD_OK;
}
int ald_batch_run(ald_batch *b)
{
    if(!b) return ALD_ERR_INVALID;
    if(!b->uploaded) return ald_set_err(ALD_ERR_STATE, "ald_batch_run before ald_batch_upload");
    int code; if(injected(E_RUN, code)) return code;
    device_delay(b->device, g_calls[E_RUN].load());
    if(S(b)->pending) { emu_result_free(S(b)->pending); S(b)->pending = nullptr; }
    int rc;
    { std::lock_guard<std::mutex> lk(g_emu); rc = emu_run_batch(b->hb, &S(b)->abi_prm, 0, -1, &S(b)->pending); }
    if(rc != ALD_OK) return ald_set_err(rc, "the emulation refused the batch");
    b->ran = true;
    return ALD_OK;
}
int ald_batch_download(ald_batch *b)
{
    if(!b) return ALD_ERR_INVALID;
    if(!b->ran || !S(b)->pending) return ald_set_err(ALD_ERR_STATE, "ald_batch_download before ald_batch_run");
    int code; if(injected(E_DOWNLOAD, code)) return code;
    device_delay(b->device, g_calls[E_DOWNLOAD].load());
    b->res = std::move(S(b)->pending->R);
    emu_result_free(S(b)->pending); S(b)->pending = nullptr;
    b->downloaded = true;
    return ALD_OK;
}

int ald_batch_get_result(const ald_batch *b, int32_t graph, ald_result_view *out)
{
    if(!b || !out || !b->downloaded || graph < 0 || graph >= b->hb.n()) return ALD_ERR_INVALID;
    out->status = b->res.status[graph]; out->num_paths = (int32_t)(b->res.path_begin[graph + 1] - b->res.path_begin[graph]);
    out->num_iterations = b->res.n_iters[graph]; out->reserved = 0;
    return ALD_OK;
}
int ald_batch_get_transcript(const ald_batch *b, int32_t graph, int32_t path, ald_transcript_view *out)
{
    if(!b || !out || !b->downloaded || graph < 0 || graph >= b->hb.n()) return ALD_ERR_INVALID;
    int64_t i = b->res.path_begin[graph] + path;
    if(path < 0 || i >= b->res.path_begin[graph + 1]) return ALD_ERR_INVALID;
    const PathRec p = b->res.path(i);
    out->num_exons = p.nexw / 2; out->exons = b->res.exons(p);
    out->coverage = p.coverage; out->conf = p.conf; out->abd = p.abd; out->count1 = p.count; out->strand = p.strand;
    return ALD_OK;
}

int ald_tset_add_batch(ald_tset *t, const ald_batch *b, const int32_t *sid, int64_t tid_base, int32_t skip_single_exon)
{
    int code; if(injected(E_MERGE, code)) return code;
    const long before = thread_probe().peak; thread_probe().peak = 0;
    const int rc = ald_real_tset_add_batch(t, b, sid, tid_base, skip_single_exon);
    note_min(g_sink_width_min, (int)thread_probe().peak + 1); thread_probe().peak = std::max(before, thread_probe().peak);
    return rc;
}

} // extern "C"
