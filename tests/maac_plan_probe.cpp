// CPU probe of the engine plan and the learn plan for FRL_ALGO_MAAC (csrc/engine_plan.hpp, csrc/learn_plan.hpp: plain C++, no device).
//     maac_plan_probe algo n_agents obs_dim act_dim hidden discrete n_learners batch_max   ->  one JSON line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/freerl_hip.h"
#include "frl_desc.h"
#include "learn_plan.hpp"

using namespace frl;

int main(int argc, char** argv) {
    if (argc < 9) return 2;
    frl_config c;
    memset(&c, 0, sizeof c);
    c.algo = atoi(argv[1]);
    c.n_agents = atoi(argv[2]);
    for (int j = 0; j < c.n_agents && j < FRL_MAX_AGENTS; ++j) { c.obs_dim[j] = atoi(argv[3]); c.act_dim[j] = atoi(argv[4]); }
    c.hidden = atoi(argv[5]);
    c.discrete = atoi(argv[6]);
    c.n_learners = atoi(argv[7]); c.capacity = 256; c.batch_max = atoi(argv[8]); c.hidden_act = FRL_ACT_LEAKY_RELU;
    EnginePlan pl;
    std::string why;
    if (plan_engine(c, nullptr, PlanLimits(), PlanKnobs(), &pl, &why) != FRL_OK) {
        printf("{\"refused\": 1, \"message\": \"%s\"}\n", why.c_str());
        return 0;
    }
    const EngineDesc& h = pl.h;
    printf("{\"refused\": 0, \"algo\": %d, \"desc_algo\": %d, \"rc\": %d, \"cps\": %d, \"lds_bytes\": %d, \"lds_budget\": %d, \"n_nets\": %d, \"learn\": \"%s\", ", (int)FRL_ALGO_MAAC,
           (int)ALGO_MAAC, h.rc, h.cps, pl.lds_bytes, family_lds_bytes(pl.family, 8), h.n_nets, algo_traits(c.algo).learn);
    printf("\"maac_off\": %d, \"att_size\": %d, \"learner_stride\": %d, \"noise_sets\": %d, \"alpha_count\": %zu, \"act_dim\": %d, ", h.maac_off, h.maac_att.size,
           h.learner_stride, h.noise_sets, pl.alpha_count, h.rec.act_dim[0]);
    for (int net = 0; net < 2; ++net) {
        printf("\"layers%d\": [", net);
        for (int l = 0; l < h.net[net].n_layers; ++l) printf("%s[%d, %d]", l ? ", " : "", h.net[net].L[l].n, h.net[net].L[l].k);
        printf("], ");
    }
    printf("\"att_layers\": [");
    for (int l = 0; l < h.maac_att.n_layers; ++l) printf("%s[%d, %d]", l ? ", " : "", h.maac_att.L[l].n, h.maac_att.L[l].k);
    // the learn plan of one device-drawn call: (stage, agent, draw) per launch
    LearnFacts F;
    F.h = &h; F.f = &pl; F.min_size = 256;
    frl_learn_args a;
    memset(&a, 0, sizeof a);
    a.batch = 1;
    LearnPlan lp;
    std::vector<int> narrowed;
    const int rc = plan_learn(F, LearnKnobs(), a, LEARN_PLAIN, &lp, &narrowed, &why);
    printf("], \"learn_rc\": %d, \"launches\": [", rc);
    for (int i = 0; rc == FRL_OK && i < lp.n_launches; ++i) printf("%s[%d, %d, %d]", i ? ", " : "", lp.launches[i].stage, lp.launches[i].agent, (int)lp.launches[i].draw);
    printf("]}\n");
    return 0;
}
