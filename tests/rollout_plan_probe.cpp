// Stand-alone probe of csrc/rollout_plan.hpp (tests/test_rollout_plan.py compiles it with g++ -fsanitize=address,undefined — no hipcc,
// which is the proof that the header is free of HIP — and runs it): what a frl_rollout call decides before it touches the device.  The
// expected values are the rules as the project documents them ("the rollout loop's step folded into the launches" and
// "pre-armed launches on two streams"; include/freerl_hip.h: frl_rollout_args), written out as literals.  "rollout_plan ok", or the
// first violated line and a non-zero exit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rollout_plan.hpp"

using namespace frl;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            printf("rollout_plan_probe.cpp:%d: %s\n", __LINE__, #cond);        \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

// a DQN engine on the one-launch update (8 observations, 4 actions) over a matching discrete pool of P x E envs
static RolloutFacts dqn_facts(int P, int E = 1) {
    RolloutFacts f;
    f.algo = ALGO_DQN; f.P = P; f.capacity = 1000; f.n_discrete = 4; f.rec_obs_dim = 8; f.rec_act_dim = 1;
    f.family = FAM_DQN_FUSED;
    f.n = P * E; f.obs_dim = 8; f.act_dim = 1; f.n_actions = 4; f.discrete = true; f.max_action = 0.f;
    f.blk_bytes = BlkLayout(P, P * E, 8).bytes;
    return f;
}
// a TD3 / SAC / DDPG engine on the single-learner kernels (sixteen workgroups per learner) over a continuous pool, max_action 2
static RolloutFacts solo_facts(int algo, int P, int E = 1) {
    RolloutFacts f;
    f.algo = algo; f.P = P; f.capacity = 1000; f.rec_obs_dim = 8; f.rec_act_dim = 2; f.solo = 16;
    f.family = FAM_SOLO;
    f.n = P * E; f.obs_dim = 8; f.act_dim = 2; f.max_action = 2.f;
    f.blk_bytes = BlkLayout(P, P * E, 8).bytes;
    return f;
}
static frl_rollout_args args(int E = 1) {
    frl_rollout_args a;
    memset(&a, 0, sizeof a);
    a.n_steps = 100; a.envs_per_learner = E; a.start_steps = 64; a.learn_every = 1; a.learn.batch = 32;
    return a;
}
static RolloutPlan planned(const RolloutFacts& f, const RolloutKnobs& k, const frl_rollout_args& a) {
    RolloutPlan pl;
    std::string why;
    const int rc = plan_rollout(f, k, a, &pl, &why);
    if (rc != FRL_OK) { printf("refused: %s\n", why.c_str()); exit(1); }
    return pl;
}
static RolloutPlan planned(const RolloutFacts& f, const RolloutKnobs& k = RolloutKnobs()) { return planned(f, k, args(f.n / f.P)); }
static void refused(const RolloutFacts& f, const frl_rollout_args& a, int code, const char* text, int line) {
    RolloutPlan pl;
    std::string why;
    const int rc = plan_rollout(f, RolloutKnobs(), a, &pl, &why);
    if (rc != code || why != text) { printf("rollout_plan_probe.cpp:%d: code %d \"%s\", expected %d \"%s\"\n", line, rc, why.c_str(), code, text); exit(1); }
}
#define REFUSED(f, a, code, text) refused(f, a, code, text, __LINE__)

static void arming() {
    RolloutKnobs on, off;
    on.prearm = 1; off.prearm = 0;
    // DQN on the fold: armed by default up to 32 learners; FRL_ROLLOUT_PREARM=1 past them, =0 nowhere
    RolloutPlan p = planned(dqn_facts(32));
    CHECK(p.fold == FOLD_DQN && p.zero_copy && p.poll && p.prearm && p.dev && !p.host_commit);
    CHECK(planned(dqn_facts(1)).prearm);
    CHECK(!planned(dqn_facts(33)).prearm && planned(dqn_facts(33)).fold == FOLD_DQN && planned(dqn_facts(33)).poll);
    CHECK(planned(dqn_facts(33), on).prearm);
    CHECK(!planned(dqn_facts(32), off).prearm && !planned(dqn_facts(1), off).prearm && !planned(dqn_facts(33), off).prearm);
    // the solo fold: up to two learners
    p = planned(solo_facts(ALGO_TD3, 2));
    CHECK(p.fold == FOLD_SOLO && p.zero_copy && p.poll && p.prearm);
    CHECK(!planned(solo_facts(ALGO_TD3, 3)).prearm && planned(solo_facts(ALGO_TD3, 3)).fold == FOLD_SOLO);
    CHECK(planned(solo_facts(ALGO_SAC, 1)).prearm && planned(solo_facts(ALGO_DDPG, 2)).prearm);
    CHECK(!planned(solo_facts(ALGO_TD3, 2), off).prearm);
    // forced: an armed solo launch must fit next to the running one, 2 x 16 workgroups per learner on 256 CUs
    CHECK(planned(solo_facts(ALGO_TD3, 3), on).prearm);
    CHECK(planned(solo_facts(ALGO_TD3, 8), on).prearm);        // 8 * 2 * 16 = 256
    CHECK(!planned(solo_facts(ALGO_TD3, 9), on).prearm);       // 288
    RolloutFacts f = solo_facts(ALGO_TD3, 20);
    f.solo = 8;                                                 // (17 .. 32 learners: eight workgroups each) 20 * 2 * 8 = 320
    CHECK(!planned(f, on).prearm);
    f = solo_facts(ALGO_TD3, 2);
    f.n_cus = 63;                                               // a partitioned device: 2 * 2 * 16 = 64 do not fit
    CHECK(!planned(f).prearm && planned(f).poll);
    f = dqn_facts(40);
    f.n_cus = 8;                                                // (the DQN launch does not need every workgroup resident)
    CHECK(planned(f, on).prearm);
    // forcing arms nothing that is not folded and flagged
    RolloutKnobs k = on;
    k.poll = false;
    CHECK(!planned(dqn_facts(1), k).prearm && !planned(dqn_facts(1), k).poll && planned(dqn_facts(1), k).zero_copy);
    k = RolloutKnobs();
    k.poll = false;                                             // FRL_ROLLOUT_POLL=0
    CHECK(!planned(dqn_facts(1), k).prearm && !planned(solo_facts(ALGO_TD3, 1), k).prearm);
    k = on;
    k.dqn_step_fuse = false;
    CHECK(!planned(dqn_facts(1), k).prearm && planned(dqn_facts(1), k).fold == FOLD_NONE && !planned(dqn_facts(1), k).poll);
    CHECK(planned(solo_facts(ALGO_TD3, 1), k).fold == FOLD_SOLO);      // (each switch its own fold)
    k = on;
    k.solo_step_fuse = false;
    CHECK(planned(solo_facts(ALGO_TD3, 1), k).fold == FOLD_NONE && !planned(solo_facts(ALGO_TD3, 1), k).prearm && planned(dqn_facts(1), k).fold == FOLD_DQN);
    // a profiled engine arms nothing (its launches are timed one by one), forced or not
    f = dqn_facts(1);
    f.profile = true;
    CHECK(!planned(f).prearm && !planned(f, on).prearm && planned(f).fold == FOLD_DQN && planned(f).poll);
    // the patience with an armed launch: one second, FRL_ROLLOUT_ARM_PATIENCE_MS in milliseconds
    CHECK(planned(dqn_facts(1)).arm_patience == 1.0);
    k = RolloutKnobs();
    k.arm_patience_ms = 0.0;
    CHECK(planned(dqn_facts(1), k).arm_patience == 0.0);
    k.arm_patience_ms = 250.0;
    CHECK(planned(dqn_facts(1), k).arm_patience == 0.25);
    k.timing = true;
    CHECK(planned(dqn_facts(1), k).timing && !planned(dqn_facts(1)).timing);
}

static void folds_and_copies() {
    // the solo fold takes up to 1024 envs per learner
    RolloutFacts f = solo_facts(ALGO_DDPG, 1, 1024);
    f.capacity = 4096;
    CHECK(planned(f).fold == FOLD_SOLO);
    f = solo_facts(ALGO_DDPG, 1, 1025);
    f.capacity = 4096;
    CHECK(planned(f).fold == FOLD_NONE && !planned(f).poll && !planned(f).prearm);
    f = dqn_facts(1, 1025);                                     // (the DQN fold has no such bound)
    f.capacity = 4096;
    CHECK(planned(f).fold == FOLD_DQN);
    // blocks of up to 64 KiB are read in place; FRL_ROLLOUT_ZEROCOPY overrides both ways
    RolloutKnobs zc0, zc1;
    zc0.zero_copy = 0; zc1.zero_copy = 1;
    f = dqn_facts(1);
    f.blk_bytes = 65536;
    CHECK(planned(f).zero_copy && planned(f).poll && planned(f).prearm);
    CHECK(!planned(f, zc0).zero_copy && !planned(f, zc0).poll && !planned(f, zc0).prearm && planned(f, zc0).fold == FOLD_DQN);
    f.blk_bytes = 65552;
    CHECK(!planned(f).zero_copy && !planned(f).poll && !planned(f).prearm && planned(f).fold == FOLD_DQN);
    CHECK(planned(f, zc1).zero_copy && planned(f, zc1).poll && planned(f, zc1).prearm);
    // a PER engine's records go through the staged add path: nothing on the device side of the step
    f = dqn_facts(2);
    f.per_on = true;
    frl_rollout_args a = args();
    a.learn.per = 1;
    RolloutKnobs all;
    all.zero_copy = 1; all.prearm = 1;
    for (const RolloutKnobs& k : {RolloutKnobs(), all}) {
        const RolloutPlan p = planned(f, k, a);
        CHECK(p.dev && p.host_commit && p.fold == FOLD_NONE && !p.zero_copy && !p.poll && !p.prearm);
    }
    // host_explore = 1: round 1's loop
    a = args();
    a.host_explore = 1;
    for (const RolloutFacts& g : {dqn_facts(1), solo_facts(ALGO_TD3, 1), solo_facts(ALGO_SAC, 2)})
        for (const RolloutKnobs& k : {RolloutKnobs(), all}) {
            const RolloutPlan p = planned(g, k, a);
            CHECK(!p.dev && p.host_commit && p.fold == FOLD_NONE && !p.zero_copy && !p.poll && !p.prearm);
        }
    // the fold follows the family of the call's frl_learn: a DQN engine with FRL_DQN_FUSED off, a solo engine at a batch past 256 or with
    // Batch_ObsNorm on (row-chunk kernels), the chained family
    f = dqn_facts(1);
    f.family = FAM_ROWCHUNK;
    CHECK(planned(f).fold == FOLD_NONE && planned(f).zero_copy && !planned(f).poll && !planned(f, all).prearm);
    f = solo_facts(ALGO_TD3, 1);
    f.family = FAM_ROWCHUNK;
    CHECK(planned(f).fold == FOLD_NONE && !planned(f, all).prearm);
    f.family = FAM_CHAINED;
    CHECK(planned(f).fold == FOLD_NONE);
    f.family = FAM_DQN_FUSED;                                   // (no such engine; the families are asked for by algorithm)
    CHECK(planned(f).fold == FOLD_NONE);
    f = dqn_facts(1);
    f.family = FAM_SOLO;
    CHECK(planned(f).fold == FOLD_NONE);
}

static void exploration() {
    // explore_kind 0 (a zero-initialised struct) and -1: the reference loop's own rule per algorithm
    for (int dflt : {0, -1}) {
        frl_rollout_args a = args();
        a.explore_kind = dflt;
        RolloutPlan p = planned(dqn_facts(1), RolloutKnobs(), a);
        CHECK(p.kind == FRL_EXPLORE_EPS_GREEDY && p.mode == FRL_ACT_ARGMAX && p.aout == 1 && p.ma == 1.f);
        p = planned(solo_facts(ALGO_SAC, 1), RolloutKnobs(), a);
        CHECK(p.kind == FRL_EXPLORE_NONE && p.mode == FRL_ACT_SAC_SAMPLE && p.aout == 2 && p.ma == 2.f);
        p = planned(solo_facts(ALGO_TD3, 1), RolloutKnobs(), a);
        CHECK(p.kind == FRL_EXPLORE_GAUSS && p.mode == FRL_ACT_TANHHEAD && p.aout == 2 && p.ma == 2.f);
        CHECK(planned(solo_facts(ALGO_DDPG, 1), RolloutKnobs(), a).kind == FRL_EXPLORE_GAUSS);
    }
    frl_rollout_args a = args();
    a.explore_kind = FRL_EXPLORE_OFF;
    CHECK(planned(solo_facts(ALGO_TD3, 1), RolloutKnobs(), a).kind == FRL_EXPLORE_NONE);
    a.explore_kind = FRL_EXPLORE_OU;
    CHECK(planned(solo_facts(ALGO_DDPG, 1), RolloutKnobs(), a).kind == FRL_EXPLORE_OU);
    a.explore_kind = FRL_EXPLORE_GAUSS;
    CHECK(planned(solo_facts(ALGO_SAC, 1), RolloutKnobs(), a).kind == FRL_EXPLORE_GAUSS);
    a.explore_kind = FRL_EXPLORE_EPS_GREEDY;
    CHECK(planned(dqn_facts(1), RolloutKnobs(), a).kind == FRL_EXPLORE_EPS_GREEDY);
}

static void refusals() {
    // every refusal once, in the order frl_rollout states them
    RolloutFacts f = dqn_facts(2, 2);
    f.n = 6;
    REFUSED(f, args(2), FRL_ERR_INVALID, "pool has 6 envs, engine needs P*E = 2*2");
    REFUSED(dqn_facts(2, 2), args(0), FRL_ERR_INVALID, "pool has 4 envs, engine needs P*E = 2*0");
    f = dqn_facts(1, 5);
    f.capacity = 4;
    REFUSED(f, args(5), FRL_ERR_INVALID, "a vector step adds E = 5 rows to a ring of 4");
    f = dqn_facts(1);
    f.rec_obs_dim = 7;
    REFUSED(f, args(), FRL_ERR_INVALID, "obs_dim mismatch (8 vs 7)");
    f = dqn_facts(1);
    f.discrete = false;
    REFUSED(f, args(), FRL_ERR_INVALID, "DQN needs a discrete env and the others a continuous one");
    f = solo_facts(ALGO_TD3, 1);
    f.discrete = true;
    REFUSED(f, args(), FRL_ERR_INVALID, "DQN needs a discrete env and the others a continuous one");
    f = solo_facts(ALGO_TD3, 1);
    f.act_dim = 3;
    REFUSED(f, args(), FRL_ERR_INVALID, "act_dim mismatch");
    f = dqn_facts(1);
    f.n_actions = 3;
    REFUSED(f, args(), FRL_ERR_INVALID, "n_actions mismatch");
    static const int64_t some_idx[1] = {0};
    static const float some_noise[1] = {0.f};
    frl_rollout_args a = args();
    a.learn.idx = some_idx;
    REFUSED(dqn_facts(1), a, FRL_ERR_INVALID, "rollout draws on the device: learn.idx/noise must be NULL");
    a = args();
    a.learn.noise = some_noise;
    REFUSED(solo_facts(ALGO_TD3, 1), a, FRL_ERR_INVALID, "rollout draws on the device: learn.idx/noise must be NULL");
    f = dqn_facts(1);
    f.per_on = true;
    REFUSED(f, args(), FRL_ERR_STATE, "PER engine: set learn.per (1 reference weighting, 2 per-sample) so the rollout samples and updates priorities");
    a = args();
    a.learn_every = 0;                                          // (collecting only needs no priorities)
    CHECK(planned(f, RolloutKnobs(), a).host_commit);
    a = args();
    a.learn.per = 1;
    REFUSED(dqn_facts(1), a, FRL_ERR_STATE, "learn.per needs frl_per_enable");
    a = args();
    a.explore_kind = FRL_EXPLORE_OFF + 1;
    REFUSED(solo_facts(ALGO_TD3, 1), a, FRL_ERR_INVALID, "unknown exploration kind 5");
    a.explore_kind = FRL_EXPLORE_EPS_GREEDY;
    REFUSED(solo_facts(ALGO_TD3, 1), a, FRL_ERR_INVALID, "epsilon-greedy is the discrete rule, Gaussian / OU / none the continuous ones");
    a.explore_kind = FRL_EXPLORE_GAUSS;
    REFUSED(dqn_facts(1), a, FRL_ERR_INVALID, "epsilon-greedy is the discrete rule, Gaussian / OU / none the continuous ones");
    a.explore_kind = FRL_EXPLORE_OFF;
    REFUSED(dqn_facts(1), a, FRL_ERR_INVALID, "epsilon-greedy is the discrete rule, Gaussian / OU / none the continuous ones");
    a.explore_kind = FRL_EXPLORE_OU;
    a.host_explore = 1;
    REFUSED(solo_facts(ALGO_DDPG, 1), a, FRL_ERR_INVALID, "OU exploration runs on the device path only");
    // the order: of two faults the one stated first is reported
    f = dqn_facts(2, 2);
    f.n = 6; f.rec_obs_dim = 7;
    REFUSED(f, args(2), FRL_ERR_INVALID, "pool has 6 envs, engine needs P*E = 2*2");
    f = dqn_facts(1);
    f.rec_obs_dim = 7; f.n_actions = 3;
    a = args();
    a.learn.per = 1;
    REFUSED(f, a, FRL_ERR_INVALID, "obs_dim mismatch (8 vs 7)");
    f = dqn_facts(1);
    f.n_actions = 3;
    REFUSED(f, a, FRL_ERR_INVALID, "n_actions mismatch");
    a.explore_kind = FRL_EXPLORE_OFF + 1;
    REFUSED(dqn_facts(1), a, FRL_ERR_STATE, "learn.per needs frl_per_enable");
}

static void block_layout() {
    // [scale P f32 | row n i32 | next_obs n*O | obs_next n*O | reward n | flags n u8], sections 16-byte aligned
    const BlkLayout l(3, 6, 5);
    CHECK(l.off_row == 16 && l.off_nobs == 48 && l.off_onext == 176 && l.off_rew == 304 && l.off_flags == 336 && l.bytes == 352);
    static unsigned char base[352];
    const BlkView v = l.view(base);
    CHECK((unsigned char*)v.scale == base && (unsigned char*)v.row == base + 16 && (unsigned char*)v.next_obs == base + 48);
    CHECK((unsigned char*)v.obs_next == base + 176 && (unsigned char*)v.reward == base + 304 && v.flags == base + 336);
    const BlkLayout one(1, 1, 1);
    CHECK(one.off_row == 16 && one.off_nobs == 32 && one.off_onext == 48 && one.off_rew == 64 && one.off_flags == 80 && one.bytes == 96);
    CHECK(BlkLayout(4, 4, 4).off_row == 16 && BlkLayout(5, 4, 4).off_row == 32);
}

static void learn_steps() {
    // frl_rollout_args: learn once every ring holds MORE rows than start_steps, every learn_every vector steps, and the device draw
    // needs 2 * batch rows
    frl_rollout_args a = args();
    a.start_steps = 0; a.learn.batch = 32;
    a.learn_every = 0;
    CHECK(!learn_due(a, 0, 1000) && !learn_due(a, 7, 1000));
    a.learn_every = 3;
    CHECK(!learn_due(a, 0, 1000) && !learn_due(a, 1, 1000) && learn_due(a, 2, 1000) && !learn_due(a, 3, 1000) && learn_due(a, 5, 1000));
    a.learn_every = 1;
    CHECK(!learn_due(a, 0, 63) && learn_due(a, 0, 64));         // 2 * batch - 1 against 2 * batch
    a.start_steps = 200;
    CHECK(!learn_due(a, 0, 200) && learn_due(a, 0, 201));       // min_size == start_steps
    a.learn.batch = 128;
    CHECK(!learn_due(a, 0, 255) && learn_due(a, 0, 256));
}

int main() {
    arming();
    folds_and_copies();
    exploration();
    refusals();
    block_layout();
    learn_steps();
    printf("rollout_plan ok\n");
    return 0;
}
