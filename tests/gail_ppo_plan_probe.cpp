// CPU probe of the engine plan for FRL_ALGO_GAIL_PPO (csrc/engine_plan.hpp: plain C++, no device) and of what every OTHER algorithm's
// plan says to the configuration that is this one's own: the walk over algorithms of tests/engine_plan_probe.cpp, extended by one.
//     gail_ppo_plan_probe name algo obs act hidden batch_max n_learners discrete hidden_act extra_cols capacity   ->  one JSON line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/freerl_hip.h"
#include "frl_desc.h"
#include "engine_plan.hpp"

using namespace frl;

int main(int argc, char** argv) {
    if (argc < 12) return 2;
    int a = 1;
    const char* name = argv[a++];
    frl_config c;
    memset(&c, 0, sizeof c);
    c.n_agents = 1;
    c.algo = atoi(argv[a++]);
    c.obs_dim[0] = atoi(argv[a++]);
    c.act_dim[0] = atoi(argv[a++]);
    c.hidden = atoi(argv[a++]);
    c.batch_max = atoi(argv[a++]);
    c.n_learners = atoi(argv[a++]);
    c.discrete = atoi(argv[a++]);
    c.hidden_act = atoi(argv[a++]);
    c.extra_cols = atoi(argv[a++]);
    c.capacity = atoi(argv[a++]);
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
    const AlgoTraits& T = algo_traits(c.algo);
    printf("{\"name\": \"%s\", \"algo_name\": \"%s\", \"learn\": \"%s\", \"act_hint\": \"%s\", \"rollout\": %d, \"n_nets\": %d, \"family\": %d, \"row_chunk\": %d, "
           "\"lds_bytes\": %d, \"lds_for_rc\": %d, \"cps\": %d, \"S\": %d, \"n_discrete\": %d, \"cat_logits\": %d, \"log_std_min\": %g, \"log_std_max\": %g, "
           "\"width\": %d, \"stride\": %d, \"act_cols\": %d, \"extra\": %d, \"done_off\": %d, \"rew_off\": %d, \"lds_act_pad\": %d, \"lds_out_pad\": %d, \"lds_kin_pad\": %d, "
           "\"learner_stride\": %d, \"nets\": [",
           name, T.name, T.learn, T.act_hint, (int)T.rollout, h.n_nets, (int)pl.family, h.rc, pl.lds_bytes, lds_bytes_for(h, h.rc), h.cps, h.S, h.n_discrete,
           h.cat_logits, (double)h.log_std_min, (double)h.log_std_max, h.rec.width, h.rec.stride, h.rec.act_dim[0], h.rec.extra, h.rec.done_off, h.rec.rew_off,
           h.lds_act_pad, h.lds_out_pad, h.lds_kin_pad, h.learner_stride);
    for (int i = 0; i < h.n_nets; ++i) {
        const NetDesc& N = h.net[i];
        printf("%s{\"heads\": %d, \"extra_n\": %d, \"extra_off\": %d, \"size\": %d, \"out_act\": %d, \"hidden_act\": %d, \"layers\": [", i ? ", " : "", N.heads, N.extra_n,
               N.extra_off, N.size, N.out_act, N.hidden_act);
        for (int l = 0; l < N.n_layers; ++l) printf("%s[%d, %d]", l ? ", " : "", N.L[l].n, N.L[l].k);
        printf("]}");
    }
    printf("]}\n");
    return 0;
}
