// CPU probe of plan_popart_ddpg (csrc/learn_plan.hpp) and of the learner block's layout (csrc/rowchunk_layout.h) on two learners of (3, 2), hidden 32.
//     popart_plan_probe call batch_max batch size0 size1 beta use_idx idx_value   ->  {"rc", "message", "rows", "ns"}
//     popart_plan_probe walk batch_max rc cps                                     ->  {"ok", "stride", "S"}: no two regions of a block overlap
#include <cstdlib>

#include "learn_plan.hpp"

using namespace frl;

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    frl_config c;
    memset(&c, 0, sizeof c);
    c.algo = FRL_ALGO_DDPG_POPART; c.n_learners = 2; c.n_agents = 1; c.obs_dim[0] = 3; c.act_dim[0] = 2; c.hidden = 32; c.hidden_act = FRL_ACT_RELU;
    c.capacity = 40; c.batch_max = atoi(argv[2]);
    PlanKnobs knobs;
    const bool walk = !strcmp(argv[1], "walk");
    if (walk) { knobs.rc = atoi(argv[3]); knobs.cps = atoi(argv[4]); }
    EnginePlan pl;
    std::string why;
    if (plan_engine(c, nullptr, PlanLimits(), knobs, &pl, &why) != FRL_OK) { printf("{\"rc\": 1, \"message\": \"%s\"}\n", why.c_str()); return 0; }
    const EngineDesc& h = pl.h;
    if (walk) {
        bool ok = h.popart_stride % 2 == 0 && pl.popart_count == (size_t)h.P * h.popart_stride && rowchunk_ns(h, h.batch_max) <= h.S;
        for (int p = 0; p < h.P; ++p) {
            const size_t lo = popart_offset(h, p), hi = popart_offset(h, p + 1);
            ok = ok && popart_part_offset(h, p, 0) == lo + kPopartHead && POP_STEP < kPopartHead && popart_part_offset(h, p, 0) % 2 == 0;
            ok = ok && popart_part_offset(h, p, h.S - 1) + kPopartPart == popart_y_offset(h, p, 0) && popart_y_offset(h, p, h.batch_max - 1) < hi;
        }
        printf("{\"ok\": %d, \"stride\": %d, \"S\": %d}\n", (int)ok, h.popart_stride, h.S);
        return 0;
    }
    if (argc < 9) return 2;
    frl_popart_ddpg_args a;
    memset(&a, 0, sizeof a);
    a.batch = atoi(argv[3]);
    a.gamma = 0.99f; a.tau = 0.01f; a.actor_lr = a.critic_lr = a.upper_lr = 1e-3f; a.beta = (float)atof(argv[6]);
    const int sizes[2] = {atoi(argv[4]), atoi(argv[5])};
    std::vector<int64_t> idx((size_t)2 * h.batch_max, atoll(argv[8]));
    if (atoi(argv[7])) a.idx = idx.data();
    PopartPlan pp;
    std::vector<int> narrow;
    const int rc = plan_popart_ddpg(h, sizes, a, &pp, &narrow, &why);
    printf("{\"rc\": %d, \"message\": \"%s\", \"rows\": %d, \"ns\": %d}\n", rc, why.c_str(), pp.rows, pp.ns);
    return 0;
}
