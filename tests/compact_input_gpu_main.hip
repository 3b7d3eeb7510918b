// compact_input_gpu_main.hip -- GPU tier of the compact-input tests: the expand kernels of aletsch_amd/csrc/input_expand.h against the
// host's staging, byte for byte, on every case of compact_input_cases.h.  Built by tests/test_compact_input_gpu.py
// (hipcc --offload-arch=gfx950) and run once.  For a case:
//   * an eager batch is staged and its section bytes kept;
//   * a compact batch is staged; the device buffer is filled with a pattern, the sections that travel are copied, the per-graph sample
//     ids go up, the expand kernels run, the whole buffer comes back;
//   * every section -- derived or sent -- must hold the eager batch's bytes, and every byte between sections must still hold the pattern
//     (nothing is written outside a section).
// One line per case ("ok" / "FAIL" + the sections that differ); exit status 1 if any case failed, 2 on a HIP error.
#include "../aletsch_amd/csrc/input_expand.h"
#include "compact_input_cases.h"
#include <cstdio>
#include <cstdlib>

using namespace cic;
typedef HostBatch::Section Sec;
#define CHK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { printf("HIP error: %s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while(0)

int main()
{
    int ndev = 0;
    if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { printf("no HIP device\n"); return 2; }
    hipStream_t st; CHK(hipStreamCreate(&st));
    int failures = 0;
    for(const Case &c : cases()) {
        HostBatch E, C; C.compact = true;
        if(stage(E, c, true) != ALD_OK || stage(C, c, true) != ALD_OK) { printf("FAIL %s: staging\n", c.name.c_str()); failures++; continue; }
        Sec se[HostBatch::S_COUNT], sc[HostBatch::S_COUNT];
        const uint64_t be = E.layout(se), bc = C.layout(sc);
        bool same_layout = be == bc;
        for(int i = 0; i < HostBatch::S_COUNT; i++) same_layout = same_layout && se[i].off == sc[i].off && se[i].bytes == sc[i].bytes;
        const unsigned derive = derive_mask(sc);
        if(!same_layout || derive != c.expect) { printf("FAIL %s: layout (derived mask %u, expected %u)\n", c.name.c_str(), derive, c.expect); failures++; continue; }
        uint8_t *d = nullptr; int32_t *d_gsid = nullptr; const int n = C.n();
        CHK(hipMalloc((void**)&d, bc)); CHK(hipMalloc((void**)&d_gsid, 4 * (size_t)n + 4));
        CHK(hipMemsetAsync(d, 0xA5, bc, st));
        uint64_t sent = 0;
        for(int i = 0; i < HostBatch::S_COUNT; i++) if(sc[i].bytes && !sc[i].derived) { CHK(hipMemcpyAsync(d + sc[i].off, sc[i].src, sc[i].bytes, hipMemcpyHostToDevice, st)); sent += sc[i].bytes; }
        CHK(hipMemcpyAsync(d_gsid, C.g_sid.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
        const BatchIn in = C.make_batch_in(d, sc);
        CHK(expand_input(in, d_gsid, C.off_v.back(), C.off_e.back(), derive, st));
        std::vector<uint8_t> back((size_t)bc);
        CHK(hipMemcpyAsync(back.data(), d, bc, hipMemcpyDeviceToHost, st));
        CHK(hipStreamSynchronize(st));
        CHK(hipFree(d)); CHK(hipFree(d_gsid));
        std::string bad; uint64_t covered = 0, full = 0;
        std::vector<uint8_t> in_section((size_t)bc, 0);
        for(int i = 0; i < HostBatch::S_COUNT; i++) {
            full += se[i].bytes;
            if(!se[i].bytes) continue;
            if(memcmp(back.data() + se[i].off, se[i].src, se[i].bytes) != 0) { bad += ' '; bad += section_name(i); bad += sc[i].derived ? "(derived)" : "(sent)"; }
            memset(in_section.data() + se[i].off, 1, se[i].bytes); covered += se[i].bytes;
        }
        uint64_t touched = 0; for(uint64_t o = 0; o < bc; o++) if(!in_section[(size_t)o] && back[(size_t)o] != 0xA5) touched++;
        if(touched) bad += " " + std::to_string(touched) + " bytes outside every section written";
        if(!bad.empty()) failures++;
        printf("%s %s: graphs %d sent %llu full %llu%s\n", bad.empty() ? "ok" : "FAIL", c.name.c_str(), n, (unsigned long long)sent, (unsigned long long)full, bad.c_str());
        (void)covered;
    }
    CHK(hipStreamDestroy(st));
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
