// compact_input_config_main.cc -- the adapter's switch for compact input (aletsch_amd/host/gpu_scallop.hpp: stage_params, which both
// gpu_scallop_batch and gpu_assembly_queue hand to ald_batch_create): a configuration with a `compact_input` member sets
// ALD_PARAM_COMPACT_INPUT with it, one without the member -- the reference's own parameters class -- never does.  C++11, as the reference builds.
#include "gpu_scallop.hpp"
#include <cstdio>

struct plain_parameters { double max_decompose_error_ratio[8]; double min_guaranteed_edge_weight; double min_transcript_coverage; int max_num_exons; };
struct compact_parameters : plain_parameters { bool compact_input; };

int main()
{
    plain_parameters p = plain_parameters(); p.max_num_exons = 10000;
    compact_parameters c = compact_parameters(); c.max_num_exons = 77;
    int bad = 0;
    if(aletsch::stage_params(p).reserved != 0) { printf("FAIL a configuration without the member set the bit\n"); bad++; }
    c.compact_input = false;
    if(aletsch::stage_params(c).reserved != 0) { printf("FAIL compact_input = false set the bit\n"); bad++; }
    c.compact_input = true;
    const ald_params q = aletsch::stage_params(c);
    if(q.reserved != ALD_PARAM_COMPACT_INPUT || q.max_num_exons != 77) { printf("FAIL compact_input = true: reserved %d\n", (int)q.reserved); bad++; }
    printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
