// CPU probe of the engine plan for FRL_ALGO_MAPPO_ATT (csrc/engine_plan.hpp: plain C++, no device).
//     mappo_att_plan_probe n_agents obs_dim obs_dim_of_the_last_agent act_dim hidden   ->  one JSON line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/freerl_hip.h"
#include "frl_desc.h"
#include "engine_plan.hpp"

using namespace frl;

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    frl_config c;
    memset(&c, 0, sizeof c);
    c.algo = FRL_ALGO_MAPPO_ATT;
    c.n_agents = atoi(argv[1]);
    for (int j = 0; j < c.n_agents && j < FRL_MAX_AGENTS; ++j) { c.obs_dim[j] = atoi(argv[j == c.n_agents - 1 ? 3 : 2]); c.act_dim[j] = atoi(argv[4]); }
    c.hidden = atoi(argv[5]);
    c.n_learners = 1; c.capacity = 256; c.batch_max = 256; c.hidden_act = FRL_ACT_RELU;
    c.extra_cols = c.n_agents * (c.act_dim[0] + 1);
    EnginePlan pl;
    std::string why;
    if (plan_engine(c, nullptr, PlanLimits(), PlanKnobs(), &pl, &why) != FRL_OK) {
        printf("{\"refused\": 1, \"message\": \"%s\"}\n", why.c_str());
        return 0;
    }
    const NetDesc& N = pl.h.net[1];
    printf("{\"refused\": 0, \"rc\": %d, \"lds_bytes\": %d, \"n_nets\": %d, \"learn\": \"%s\", \"layers\": [", pl.h.rc, pl.lds_bytes, pl.h.n_nets, algo_traits(c.algo).learn);
    for (int l = 0; l < N.n_layers; ++l) printf("%s[%d, %d]", l ? ", " : "", N.L[l].n, N.L[l].k);
    printf("]}\n");
    return 0;
}
