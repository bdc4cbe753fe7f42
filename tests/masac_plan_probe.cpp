// CPU probe of the engine plan for FRL_ALGO_MASAC (csrc/engine_plan.hpp: plain C++, no device): what tests/engine_plan_probe.cpp does
// not print — every net's layer shapes, the draw sets, the alpha / step-counter storage and the kernel family.
//     masac_plan_probe name n_agents obs.. act.. hidden batch_max n_learners discrete twin hidden_act [algo]   ->  one JSON line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/freerl_hip.h"
#include "frl_desc.h"
#include "engine_plan.hpp"

using namespace frl;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    int a = 1;
    const char* name = argv[a++];
    frl_config c;
    memset(&c, 0, sizeof c);
    c.n_agents = atoi(argv[a++]);
    if (argc < 3 + 2 * c.n_agents + 6) return 2;
    for (int j = 0; j < c.n_agents && j < FRL_MAX_AGENTS; ++j) c.obs_dim[j] = atoi(argv[a + j]);
    for (int j = 0; j < c.n_agents && j < FRL_MAX_AGENTS; ++j) c.act_dim[j] = atoi(argv[a + c.n_agents + j]);
    a += 2 * c.n_agents;
    c.hidden = atoi(argv[a++]);
    c.batch_max = atoi(argv[a++]);
    c.n_learners = atoi(argv[a++]);
    c.discrete = atoi(argv[a++]);
    c.twin_critic = atoi(argv[a++]);
    c.hidden_act = atoi(argv[a++]);
    c.algo = a < argc ? atoi(argv[a++]) : FRL_ALGO_MASAC;
    c.capacity = 512;
    EnginePlan pl;
    std::string why;
    const int rc = plan_engine(c, nullptr, PlanLimits(), PlanKnobs(), &pl, &why);
    if (rc != FRL_OK) {
        std::string esc;
        for (char ch : why) { if (ch == '"' || ch == '\\') esc += '\\'; esc += ch; }
        printf("{\"name\": \"%s\", \"refused\": %d, \"message\": \"%s\"}\n", name, rc, esc.c_str());
        return 0;
    }
    const EngineDesc& h = pl.h;
    printf("{\"name\": \"%s\", \"n_nets\": %d, \"noise_sets\": %d, \"family\": %d, \"fam_masac\": %d, \"row_chunk\": %d, \"lds_bytes\": %d, \"lds_row_extra\": %d, "
           "\"alpha_count\": %zu, \"steps_count\": %zu, \"noise_count\": %zu, \"act_max\": %d, \"learn_family\": %d, \"chained\": %d, \"nets\": [",
           name, h.n_nets, h.noise_sets, (int)pl.family, (int)FAM_MASAC, h.rc, pl.lds_bytes, h.lds_row_extra, pl.alpha_count, pl.steps_count, pl.noise_count,
           h.act_max, (int)learn_family(h, pl.family, h.batch_max, true), (int)learn_path(h, pl, learn_family(h, pl.family, h.batch_max, true), h.batch_max, 1).chained);
    for (int i = 0; i < h.n_nets; ++i) {
        const NetDesc& N = h.net[i];
        printf("%s{\"heads\": %d, \"extra_n\": %d, \"out_act\": %d, \"hidden_act\": %d, \"layers\": [", i ? ", " : "", N.heads, N.extra_n, N.out_act, N.hidden_act);
        for (int l = 0; l < N.n_layers; ++l) printf("%s[%d, %d]", l ? ", " : "", N.L[l].n, N.L[l].k);
        printf("]}");
    }
    printf("]}\n");
    return 0;
}
