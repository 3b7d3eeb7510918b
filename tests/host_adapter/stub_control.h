// stub_control.h -- TEST-ONLY: the knobs of tests/host_adapter/stub_batch_abi.cc, set by the test program (never by product code).
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
/* forget every call count, the injected failure, the delay and the observed widths */
void stub_reset(void);
/* ald_batch_run / ald_batch_download of a batch on device slot d sleep 0..max_ms milliseconds, drawn from (seed, d, call number): with
 * several device slots a batch cut later finishes first */
void stub_set_delay(unsigned seed, int max_ms);
/* the kth call (1-based) of `entry` -- "add_packed" (either form), "upload", "run", "download", "tset_add_batch" -- returns `code` and
 * sets ald_last_error() to "injected failure: <entry> call <kth>"; kth = 0 switches the injection off */
void stub_inject(const char *entry, long kth, int code);
long stub_calls(const char *entry);
/* host threads of the widest pass of the NARROWEST ald_tset_add_batch since stub_reset (0: none ran), and of the widest staging call */
int stub_sink_width_min(void);
int stub_stage_width_max(void);
#ifdef __cplusplus
}
#endif
