// Stand-alone probe of csrc/learn_plan.hpp (tests/test_learn_plan.py compiles it with g++ -fsanitize=address,undefined — no hipcc, which is
// the proof that the header is free of HIP — and runs it): what an off-policy learn call decides before it touches the device.  Engines
// are planned with plan_engine, so the kernel families are the real ones.  The expected values are written out here on their own: the
// launch counts of tests/test_gpu_learn_launches.py's CASES row by row, the refusals' codes and texts as the entry points have always
// given them and in their order of precedence, draw_kernel's LDS formula as the launchers used to compute it.  Without arguments: every
// check, then "learn_plan ok"; `idx <bound> <capacity> <size> v0 v1 ..`: narrow_idx on these entries (bound: wrap | held | pair, pair = the
// entries as ring 1's).  The first violated line and a non-zero exit otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "learn_plan.hpp"

using namespace frl;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("learn_plan_probe.cpp:%d: %s\n", __LINE__, #cond);        \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static frl_config config(int algo, std::vector<int> obs, std::vector<int> act, int P, int batch_max, bool twin = false, int hidden = 128, int capacity = 1024) {
    frl_config c;
    memset(&c, 0, sizeof c);
    c.algo = algo;
    c.n_learners = P;
    c.n_agents = (int)obs.size();
    for (size_t j = 0; j < obs.size(); ++j) { c.obs_dim[j] = obs[j]; c.act_dim[j] = act[j]; }
    c.discrete = algo == FRL_ALGO_DQN;
    c.hidden = hidden;
    c.hidden_act = FRL_ACT_RELU;
    c.twin_critic = twin;
    c.capacity = capacity;
    c.batch_max = batch_max;
    c.seed = 7;
    return c;
}
static EnginePlan planned(const frl_config& c, const PlanKnobs& knobs = PlanKnobs()) {
    EnginePlan pl;
    std::string why;
    const int rc = plan_engine(c, nullptr, PlanLimits(), knobs, &pl, &why);
    if (rc != FRL_OK) { printf("refused: %s\n", why.c_str()); exit(1); }
    return pl;
}
static frl_learn_args learn_args(int batch, bool td3_noise = false) {
    frl_learn_args a;
    memset(&a, 0, sizeof a);
    a.batch = batch; a.do_actor = 1;
    a.gamma = 0.99f; a.tau = 0.01f; a.actor_lr = a.critic_lr = 1e-3f; a.alpha_lr = 1e-4f; a.clip_norm = 0.5f;
    if (td3_noise) { a.use_policy_noise = 1; a.policy_noise = 0.2f; a.noise_clip = 0.5f; }
    return a;
}
static LearnFacts facts(const EnginePlan& pl, int min_size = 400) {
    LearnFacts F;
    F.h = &pl.h; F.f = &pl;
    F.min_size = min_size;
    F.predraw_bufs = pl.family == FAM_SOLO || pl.family == FAM_SOLOW;
    F.rng_counter = 5;
    return F;
}

// ------------------------------------------------------------------------ the launch lists: tests/test_gpu_learn_launches.py, CASES
struct Counts { int draw, grad_critic, adam_critic, grad_actor, adam_actor, soft; };
static void count(const LearnPlan& pl, Counts* n) {
    const bool rowchunk = pl.fam == FAM_ROWCHUNK || pl.fam == FAM_ATT || pl.fam == FAM_MASAC;      // the others hold their own reduce + Adam
    for (int i = 0; i < pl.n_launches; ++i) {
        const LearnLaunch& l = pl.launches[i];
        n->draw += l.draw;
        if (l.stage == 0) { n->grad_critic++; n->adam_critic += rowchunk; }
        if (l.stage == 1) { n->grad_actor++; n->adam_actor += rowchunk; }
        if (l.stage == 2) n->soft++;
    }
}
static void launches_case(const char* id, const frl_config& c, PlanKnobs ek, LearnKnobs k, frl_learn_args a, int calls, Counts want, LearnFamily fam) {
    const EnginePlan ep = planned(c, ek);
    LearnFacts F = facts(ep);
    Counts got{0, 0, 0, 0, 0, 0};
    for (int call = 0; call < calls; ++call) {
        LearnPlan pl;
        std::string why;
        const int rc = plan_learn(F, k, a, LEARN_PLAIN, &pl, nullptr, &why);
        if (rc != FRL_OK) { printf("%s: refused: %s\n", id, why.c_str()); exit(1); }
        if (pl.fam != fam) { printf("%s: family %d, expected %d\n", id, (int)pl.fam, (int)fam); exit(1); }
        CHECK(pl.a.rng_counter == F.rng_counter && pl.counters == 1 && pl.launches[0].stage == 0 && pl.launches[0].units == c.n_learners * c.n_agents);
        count(pl, &got);
        // what the entry point's bookkeeping does with the plan (frl_api_learn.inc: predraw_slots)
        F.rng_counter += pl.counters;
        if (pl.pre_multi) { F.ma_pre_valid = pl.pre_write; F.ma_pre_counter = F.rng_counter; F.ma_pre_size = pl.a.size; F.ma_pre_batch = pl.a.batch; }
    }
    if (memcmp(&got, &want, sizeof got)) {
        printf("%s: launches (%d, %d, %d, %d, %d, %d)\n", id, got.draw, got.grad_critic, got.adam_critic, got.grad_actor, got.adam_actor, got.soft);
        exit(1);
    }
}
static int launch_lists() {
    const std::vector<int> MO{6, 5, 7}, MA{2, 3, 2};
    PlanKnobs v2_0, v2_1, none;
    v2_0.critic_v2 = 0; v2_1.critic_v2 = 1;
    LearnKnobs k, no_dqn_fused, no_solow_fuse;
    no_dqn_fused.dqn_fused = 0; no_solow_fuse.solow_fuse = false;
    frl_learn_args td3 = learn_args(64, true), td3_critic = td3, plain = learn_args(64), sac = learn_args(64), td3_100 = learn_args(100, true);
    td3_critic.do_actor = 0;
    sac.target_entropy = -3.f;
    int n = 0;
#define CASE(...) launches_case(__VA_ARGS__), ++n
    CASE("td3_rowchunk", config(FRL_ALGO_TD3, {8}, {2}, 2, 64, true), v2_0, k, td3, 1, {1, 1, 1, 1, 1, 0}, FAM_ROWCHUNK);
    CASE("td3_rowchunk_critic_only", config(FRL_ALGO_TD3, {8}, {2}, 2, 64, true), v2_0, k, td3_critic, 1, {1, 1, 1, 0, 0, 0}, FAM_ROWCHUNK);
    CASE("maddpg_rowchunk", config(FRL_ALGO_MADDPG, MO, MA, 1, 64), v2_0, k, plain, 1, {1, 1, 1, 1, 1, 1}, FAM_ROWCHUNK);
    CASE("dqn_fused", config(FRL_ALGO_DQN, {4}, {2}, 1, 64), none, k, plain, 1, {0, 1, 0, 0, 0, 0}, FAM_DQN_FUSED);
    CASE("dqn_rowchunk", config(FRL_ALGO_DQN, {4}, {2}, 1, 64), none, no_dqn_fused, plain, 1, {1, 1, 1, 0, 0, 0}, FAM_ROWCHUNK);
    CASE("td3_chained", config(FRL_ALGO_TD3, {8}, {2}, 2, 100, true), v2_1, k, td3_100, 1, {1, 1, 0, 1, 0, 0}, FAM_CHAINED);
    CASE("td3_solo", config(FRL_ALGO_TD3, {8}, {2}, 1, 100, true), none, k, td3_100, 1, {0, 1, 0, 1, 0, 0}, FAM_SOLO);
    CASE("sac_solow_fused_step", config(FRL_ALGO_SAC, {40}, {3}, 1, 64, true), none, k, sac, 1, {0, 1, 0, 0, 0, 0}, FAM_SOLOW);
    CASE("sac_solow_two_launches", config(FRL_ALGO_SAC, {40}, {3}, 1, 64, true), none, no_solow_fuse, sac, 1, {0, 1, 0, 1, 0, 0}, FAM_SOLOW);
    // the one place where the HOST decides whether draw_kernel runs: the first call draws, the second takes the rows the first critic
    // launch's spare workgroups drew
    CASE("maddpg_solow_predrawn", config(FRL_ALGO_MADDPG, MO, MA, 1, 64), none, k, plain, 2, {1, 2, 0, 2, 0, 0}, FAM_SOLOW);
    CASE("matd3_solow", config(FRL_ALGO_MADDPG, MO, MA, 1, 64, true), none, k, td3, 2, {2, 2, 0, 2, 0, 0}, FAM_SOLOW);
    CASE("sac_wide", config(FRL_ALGO_SAC, {40}, {3}, 2, 64, true), v2_1, k, sac, 1, {1, 1, 0, 1, 0, 0}, FAM_WIDE);
    CASE("maddpg_wide", config(FRL_ALGO_MADDPG, MO, MA, 2, 64), v2_1, k, plain, 1, {1, 1, 0, 1, 0, 1}, FAM_WIDE);
    CASE("td3_h256_x_stationary", config(FRL_ALGO_TD3, {8}, {2}, 2, 64, true, 256), v2_1, k, td3, 1, {1, 1, 0, 1, 0, 0}, FAM_WIDE16);
#undef CASE
    return n;
}

// what else the plan fixes on those engines
static void plan_details() {
    PlanKnobs v2_1;
    v2_1.critic_v2 = 1;
    const EnginePlan chained = planned(config(FRL_ALGO_TD3, {8}, {2}, 2, 100, true), v2_1), solo = planned(config(FRL_ALGO_TD3, {8}, {2}, 1, 100, true));
    const EnginePlan sacw = planned(config(FRL_ALGO_SAC, {40}, {3}, 1, 64, true)), dqn = planned(config(FRL_ALGO_DQN, {4}, {2}, 1, 64));
    LearnKnobs k;
    LearnPlan pl;
    std::string why;
    frl_learn_args a = learn_args(100, true);
    a.adam_eps = 0.f; a.max_action = 0.f;
    // the defaults; the chained family's stagger fields and critic choice
    k.stagger = 3; k.stagger_groups = 8;
    CHECK(plan_learn(facts(chained), k, a, LEARN_PLAIN, &pl, nullptr, &why) == FRL_OK);
    CHECK(pl.a.adam_eps == 1e-8f && pl.a.max_action == 1.f && pl.a.beta1 == 0.9f && pl.a.beta2 == 0.999f && pl.a.do_actor == 1 && pl.a.use_policy_noise == 1);
    CHECK(pl.a.device_rng == 1 && pl.a.size == 400 && pl.a.batch == 100 && pl.a.p0 == 0 && pl.a.p_count == 2 && pl.a.huber == 0 && pl.a.fuse_actor == 0);
    CHECK(pl.a.stagger == 3 && pl.a.stagger_groups == 8 && pl.a.stagger_wgs == chained.n_cus && !pl.pre_touch);
    const RecordDesc& R = chained.h.rec;
    const bool aligned = R.nobs_off[0] % 4 == 0 && R.nobs_off[0] + 16 <= R.stride && R.rew_off % 2 == 0 && R.done_off == R.rew_off + 1;
    CHECK(pl.critic_nv == aligned);
    k.critic2_novec = true;
    CHECK(plan_learn(facts(chained), k, a, LEARN_PLAIN, &pl, nullptr, &why) == FRL_OK && !pl.critic_nv);
    // kernels_solo.hip: a plain call reads a slot and, with a CU to spare, has P spare workgroups write the next; a folded step does neither
    k = LearnKnobs();
    CHECK(plan_learn(facts(solo), k, a, LEARN_PLAIN, &pl, nullptr, &why) == FRL_OK && pl.fam == FAM_SOLO);
    CHECK(pl.pre_touch && pl.pre_read && pl.pre_write && !pl.pre_multi && pl.pre_extra == 1 && pl.a.stagger_wgs == 0);
    k.solo_predraw = false;
    CHECK(plan_learn(facts(solo), k, a, LEARN_PLAIN, &pl, nullptr, &why) == FRL_OK && pl.pre_touch && pl.pre_read && !pl.pre_write && pl.pre_extra == 0);
    k = LearnKnobs();
    CHECK(plan_learn(facts(solo), k, a, LEARN_FOLD_SOLO, &pl, nullptr, &why) == FRL_OK && !pl.pre_touch && pl.pre_extra == 0);
    CHECK(pl.head[0] == 1 && pl.tail[0] == 0 && pl.head[1] == 0 && pl.tail[1] == 1);
    a.do_actor = 0;
    CHECK(plan_learn(facts(solo), k, a, LEARN_FOLD_SOLO, &pl, nullptr, &why) == FRL_OK && pl.n_launches == 1 && pl.head[0] == 1 && pl.tail[0] == 1);
    // single-agent kernels_solow.hip: the helpers draw, no spare workgroups; the policy step folded into the critic launch
    frl_learn_args s = learn_args(64);
    CHECK(plan_learn(facts(sacw), k, s, LEARN_PLAIN, &pl, nullptr, &why) == FRL_OK && pl.fam == FAM_SOLOW && pl.a.fuse_actor == 1 && pl.needs_noise);
    CHECK(pl.pre_touch && pl.pre_read && pl.pre_write == (sacw.solow_wgs > sacw.solow_row_wgs) && pl.pre_extra == 0 && !pl.pre_multi);
    // the one-launch DQN update: its split, nothing in front of it
    CHECK(plan_learn(facts(dqn), k, s, LEARN_PLAIN, &pl, nullptr, &why) == FRL_OK && pl.fam == FAM_DQN_FUSED && pl.n_launches == 1);
    CHECK(pl.a.dqn_split == dqn_split_for(dqn.h, 64, 1, -1) && !pl.launches[0].draw && !pl.launches[0].obsnorm && !pl.launches[0].noisy_materialise);
    CHECK(pl.a.do_actor == 1 && pl.a.double_dqn == 0 && pl.a.use_isw == 0 && !pl.noisy);
    // MASAC: every critic in one launch, one actor launch per agent in agent order, then the targets
    frl_config mc = config(FRL_ALGO_MASAC, {6, 5, 7}, {2, 3, 2}, 2, 64, true);
    const EnginePlan masac = planned(mc);
    CHECK(plan_learn(facts(masac), k, s, LEARN_PLAIN, &pl, nullptr, &why) == FRL_OK && pl.fam == FAM_MASAC && pl.n_launches == 5 && pl.needs_noise);
    for (int i = 0; i < 5; ++i) CHECK(pl.launches[i].stage == (i == 0 ? 0 : i == 4 ? 2 : 1) && pl.launches[i].agent == (i >= 1 && i <= 3 ? i - 1 : 0) && pl.launches[i].units == 6);
    CHECK(pl.launches[0].draw && !pl.launches[1].draw);
}

// ------------------------------------------------------------------------------------------------------------------- refusals
static void expect(int rc, const std::string& why, int code, const char* text, int line) {
    if (rc != code || why != text) { printf("learn_plan_probe.cpp:%d: code %d \"%s\", expected %d \"%s\"\n", line, rc, why.c_str(), code, text); exit(1); }
}
enum { INVALID = FRL_ERR_INVALID, STATE = FRL_ERR_STATE };

// A refused plan_learn leaves *out untouched: the sentinels survive, so nothing a caller could act on was handed over
static void learn_refused(const EnginePlan& ep, LearnFacts F, frl_learn_args a, LearnFold fold, int code, const char* text, int line) {
    LearnPlan pl;
    pl.n_launches = -7; pl.counters = -7;
    std::vector<int> idx;
    std::string why;
    (void)ep;
    const int rc = plan_learn(F, LearnKnobs(), a, fold, &pl, &idx, &why);
    expect(rc, why, code, text, line);
    if (pl.n_launches != -7 || pl.counters != -7) { printf("learn_plan_probe.cpp:%d: a refused call left a plan behind\n", line); exit(1); }
}
#define LEARN_REFUSED(ep, F, a, fold, code, text) learn_refused(ep, F, a, fold, code, text, __LINE__)

static void learn_refusals() {
    const EnginePlan td3 = planned(config(FRL_ALGO_TD3, {8}, {2}, 1, 100, true)), dqn = planned(config(FRL_ALGO_DQN, {4}, {2}, 1, 64));
    const EnginePlan masac = planned(config(FRL_ALGO_MASAC, {6, 5, 7}, {2, 3, 2}, 1, 64, true));
    frl_config ac = config(FRL_ALGO_MADDPG_ATT, {6, 5, 7}, {2, 3, 2}, 1, 64);
    const EnginePlan att = planned(ac);
    frl_config cc = config(FRL_ALGO_DQN, {4}, {2}, 1, 64);
    cc.c51_atoms = 51; cc.c51_vmin = -10.f; cc.c51_vmax = 10.f;
    const EnginePlan c51 = planned(cc);
    frl_config sc = config(FRL_ALGO_SAC_DISCRETE, {4}, {3}, 1, 64, true);
    sc.discrete = 1;
    const EnginePlan sacd = planned(sc);
    frl_config big = config(FRL_ALGO_TD3, {8}, {2}, 1, 16384, true, 128, 40000);
    PlanKnobs v2_0;
    v2_0.critic_v2 = 0; v2_0.solo = 0;
    const EnginePlan wide_batch = planned(big, v2_0);
    const int64_t rows[100] = {0};
    const float noise[1] = {0.f};
    frl_learn_args a = learn_args(100, true), b;
    // each alone, with its code and text
    b = a; b.batch = 0; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "batch 0 outside [1,100]");
    b = a; b.batch = 101; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "batch 101 outside [1,100]");
    LEARN_REFUSED(td3, facts(td3, 99), a, LEARN_PLAIN, STATE, "a ring holds 99 rows < batch 100");
    b = a; b.per = 1; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, STATE, "per = 1 needs a DQN engine with frl_per_enable");
    b = learn_args(64); b.per = 1; LEARN_REFUSED(dqn, facts(dqn), b, LEARN_PLAIN, STATE, "per = 1 needs a DQN engine with frl_per_enable");
    LearnFacts per = facts(dqn);
    per.per_on = true;
    b.idx = rows; LEARN_REFUSED(dqn, per, b, LEARN_PLAIN, INVALID, "per = 1 uses the rows of the last frl_per_sample; idx must be NULL");
    LEARN_REFUSED(td3, facts(td3, 199), a, LEARN_PLAIN, STATE, "device index draw needs len(buffer) >= 2*batch (have 199); pass idx");
    b = learn_args(64); b.use_policy_noise = 1;
    LEARN_REFUSED(masac, facts(masac), b, LEARN_PLAIN, STATE, "frl_learn: MASAC has no target policy smoothing (MATD3's): use_policy_noise must be 0");
    LEARN_REFUSED(att, facts(att), b, LEARN_PLAIN, INVALID, "ATT-MADDPG has no target policy smoothing: use_policy_noise must be 0");
    b = learn_args(64); b.loss_kind = FRL_LOSS_HUBER; b.huber_delta = 1.f;
    LEARN_REFUSED(masac, facts(masac), b, LEARN_PLAIN, INVALID, "MASAC's critic loss is F.mse_loss (MASAC.py:241): no Huber variant");
    LEARN_REFUSED(c51, facts(c51), b, LEARN_PLAIN, STATE, "the Categorical head's loss is a cross-entropy: no Huber variant");
    LEARN_REFUSED(sacd, facts(sacd), b, LEARN_PLAIN, INVALID, "discrete SAC's critic loss is F.mse_loss (SAC_add_discrete.py:313-314): no Huber variant");
    b = a; b.idx = rows; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "idx given without noise: both or neither");
    int64_t bad[100] = {0};
    bad[99] = 1024;
    b = a; b.idx = bad; b.noise = noise; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "sample index 1024 out of range");
    bad[99] = -1025; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "sample index -1025 out of range");
    b = a; b.loss_kind = 2; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "unknown loss_kind 2");
    b = a; b.loss_kind = FRL_LOSS_HUBER; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "Huber loss needs huber_delta > 0");
    b.huber_delta = NAN; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "Huber loss needs huber_delta > 0");
    b = learn_args(64); LEARN_REFUSED(dqn, facts(dqn), b, LEARN_FOLD_SOLO, STATE, "step fusion needs a solo engine with device draws");
    // a draw_kernel launch whose two index arrays alone do not fit: refused in words (a batch of 10241 rows and up)
    b = learn_args(10241, true); LEARN_REFUSED(wide_batch, facts(wide_batch, 30000), b, LEARN_PLAIN, INVALID, "device index draw of 10241 rows does not fit the draw kernel's LDS; pass idx");
    LearnPlan ok;
    std::string why;
    b = learn_args(10240, true);
    CHECK(plan_learn(facts(wide_batch, 30000), LearnKnobs(), b, LEARN_PLAIN, &ok, nullptr, &why) == FRL_OK && ok.launches[0].draw && ok.draw.lds_bytes == kDrawLdsLimit);
    // the first applicable one wins, in the entry point's order: batch, ring, per, 2*batch, the algorithm's, idx without noise, idx range, loss_kind, Huber, the fold
    b = a; b.batch = 101; b.per = 1; b.loss_kind = 7; LEARN_REFUSED(td3, facts(td3, 3), b, LEARN_PLAIN, INVALID, "batch 101 outside [1,100]");
    b = a; b.per = 1; b.loss_kind = 7; LEARN_REFUSED(td3, facts(td3, 3), b, LEARN_PLAIN, STATE, "a ring holds 3 rows < batch 100");
    b = a; b.per = 1; b.idx = bad; b.loss_kind = 7; LEARN_REFUSED(td3, facts(td3, 150), b, LEARN_PLAIN, STATE, "per = 1 needs a DQN engine with frl_per_enable");
    b = a; b.loss_kind = 7; LEARN_REFUSED(td3, facts(td3, 150), b, LEARN_PLAIN, STATE, "device index draw needs len(buffer) >= 2*batch (have 150); pass idx");
    b = learn_args(64); b.use_policy_noise = 1; b.loss_kind = FRL_LOSS_HUBER; b.idx = bad;
    LEARN_REFUSED(masac, facts(masac), b, LEARN_PLAIN, STATE, "frl_learn: MASAC has no target policy smoothing (MATD3's): use_policy_noise must be 0");
    b.use_policy_noise = 0; LEARN_REFUSED(masac, facts(masac), b, LEARN_PLAIN, INVALID, "MASAC's critic loss is F.mse_loss (MASAC.py:241): no Huber variant");
    b = a; b.idx = bad; b.loss_kind = 7; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "idx given without noise: both or neither");
    b.noise = noise; LEARN_REFUSED(td3, facts(td3), b, LEARN_PLAIN, INVALID, "sample index -1025 out of range");
    b.idx = rows; LEARN_REFUSED(td3, facts(td3), b, LEARN_FOLD_SOLO, INVALID, "unknown loss_kind 7");
    b.loss_kind = FRL_LOSS_HUBER; LEARN_REFUSED(td3, facts(td3), b, LEARN_FOLD_SOLO, INVALID, "Huber loss needs huber_delta > 0");
    b.loss_kind = FRL_LOSS_MSE; LEARN_REFUSED(td3, facts(td3), b, LEARN_FOLD_SOLO, STATE, "step fusion needs a solo engine with device draws");
}

static void small_refusals() {
    std::string why;
    std::vector<int> idx;
    // ---- the envelope calls (one plan for both)
    frl_config ec = config(FRL_ALGO_ENVELOPE_DQN, {4}, {3}, 2, 64, false, 32, 40);
    ec.discrete = 1; ec.reward_dim = 2;
    const EnginePlan env = planned(ec);
    int sizes[2] = {40, 40};
    EnvelopePlan ep;
    const char* names = "gamma / tau / lr / beta";
    auto envelope = [&](EnvelopeCall c, std::initializer_list<float> scalars) { return plan_envelope(env.h, sizes, c, scalars, names, &ep, &idx, &why); };
    const int64_t rows16[32] = {0};
    int64_t bad16[32] = {0};
    bad16[31] = 40;
#define REF(call, code, text) expect(call, why, code, text, __LINE__)
    REF(envelope({0, 4, 0.99f, 0.5f, nullptr, nullptr}, {0.99f}), INVALID, "batch 0 must be >= 1");
    REF(envelope({16, 0, 0.99f, 0.5f, nullptr, nullptr}, {0.99f}), INVALID, "weight_num 0 must be >= 1");
    REF(envelope({16, 5, 0.99f, 0.5f, nullptr, nullptr}, {0.99f}), INVALID, "batch 16 x weight_num 5 = 80 rows > batch_max 64");
    REF(envelope({16, 4, 0.99f, 0.5f, nullptr, nullptr}, {0.99f, NAN}), INVALID, "gamma / tau / lr / beta is NaN");
    REF(envelope({16, 4, 0.99f, 1.5f, nullptr, nullptr}, {0.99f}), INVALID, "beta 1.5 outside [0, 1]");
    sizes[1] = 15;
    REF(envelope({16, 4, 0.99f, 0.5f, rows16, nullptr}, {0.99f}), STATE, "a ring holds 15 rows < batch 16");
    sizes[1] = 31;
    REF(envelope({16, 4, 0.99f, 0.5f, nullptr, nullptr}, {0.99f}), STATE, "device index draw needs len(buffer) >= 2*batch (have 31); pass idx");
    REF(envelope({16, 4, 0.99f, 0.5f, bad16, nullptr}, {0.99f}), INVALID, "sample index 40 out of range");
    REF(envelope({0, 0, 0.99f, 7.f, bad16, nullptr}, {NAN}), INVALID, "batch 0 must be >= 1");      // the first one wins
    REF(envelope({16, 4, 0.99f, 7.f, bad16, nullptr}, {NAN}), INVALID, "gamma / tau / lr / beta is NaN");
    CHECK(envelope({16, 4, 0.99f, 0.5f, rows16, nullptr}, {0.99f}) == FRL_OK && ep.rows == 64 && ep.ns == rowchunk_ns(env.h, 64) && !ep.dev_idx && ep.min_size == 31);
    sizes[1] = 40;
    CHECK(envelope({16, 4, 0.99f, 0.5f, nullptr, nullptr}, {0.99f}) == FRL_OK && ep.dev_idx && !ep.draw.table && ep.draw.lds_bytes == 128 && ep.draw.flag == 2);
    frl_config eb = config(FRL_ALGO_ENVELOPE_DQN, {4}, {3}, 1, 16384, false, 32, 40000);
    eb.discrete = 1; eb.reward_dim = 2;
    const EnginePlan envb = planned(eb);
    int size_b[1] = {40000};
    REF(plan_envelope(envb.h, size_b, {10241, 1, 0.99f, 0.5f, nullptr, nullptr}, {0.99f}, names, &ep, &idx, &why), INVALID,
        "device index draw of 10241 rows does not fit the draw kernel's LDS; pass idx");
    CHECK(plan_envelope(envb.h, size_b, {1024, 1, 0.99f, 0.5f, nullptr, nullptr}, {0.99f}, names, &ep, &idx, &why) == FRL_OK && ep.draw.table && ep.draw.flag == 0);

    // ---- frl_gail_learn
    frl_config gc = config(FRL_ALGO_GAIL, {3}, {1}, 2, 32, false, 32, 40);
    gc.hidden_act = FRL_ACT_LEAKY_RELU;
    const EnginePlan gail = planned(gc);
    int gs[2] = {40, 20};
    const float prow[1] = {0.f};
    frl_gail_args g, g0;
    memset(&g0, 0, sizeof g0);
    g0.n_expert = 8; g0.n_policy = 8; g0.gp = 1; g0.gp_weight = 5.f; g0.lr = 4e-4f; g0.beta1 = 0.5f; g0.beta2 = 0.9f; g0.adam_eps = 1e-8f; g0.policy_rows = prow;
    GailPlan gp;
    auto gl = [&]() { return plan_gail(gail.h, gs, g, &gp, &idx, &why); };
    g = g0; g.n_expert = 33; REF(gl(), INVALID, "n_expert 33 outside [1, batch_max 32]");
    g = g0; g.n_policy = 0; REF(gl(), INVALID, "n_policy 0 outside [1, batch_max 32]");
    g = g0; g.gp = 2; REF(gl(), INVALID, "gp 2 must be 0 or 1");
    g = g0; g.lr = NAN; REF(gl(), INVALID, "gp_weight / lr / beta1 / beta2 / adam_eps is NaN");
    g = g0; g.gp_weight = -1.f; REF(gl(), INVALID, "gp_weight -1 must be >= 0");
    g = g0; g.beta2 = 1.f; REF(gl(), INVALID, "betas (0.5, 1) outside [0, 1)");
    g = g0; g.policy_rows = nullptr; REF(gl(), INVALID, "policy_rows is NULL");
    int64_t gi[16] = {0};
    gi[15] = 20;      // learner 1 holds 20 rows
    g = g0; g.idx = gi; REF(gl(), STATE, "idx entry 20 of learner 1 is not one of its 20 stored rows");
    gs[1] = 0; REF(gl(), STATE, "a learner's ring is empty: store the expert rows first");
    g.policy_rows = nullptr; g.gp = 2; REF(gl(), INVALID, "gp 2 must be 0 or 1");      // the first one wins
    gs[1] = 21; g = g0; g.idx = gi;
    CHECK(gl() == FRL_OK && gp.min_size == 21 && gp.ns == rowchunk_ns(gail.h, 16) && idx.size() == 16 && idx[15] == 20);

    // ---- frl_cem_gd3pg_learn
    frl_config cc = config(FRL_ALGO_CEM_GD3PG, {4}, {3}, 2, 16, false, 32, 40);
    cc.hidden_act = FRL_ACT_TANH;
    const EnginePlan cem = planned(cc);
    CHECK(cem.ring_cap == 40 && cem.n_rings == 2);
    int s1[2] = {40, 9};
    const int f1[2] = {1, 0};
    float delta[2] = {0.3f, 0.3f};
    frl_cem_gd3pg_args c, c0;
    memset(&c0, 0, sizeof c0);
    c0.batch = 16; c0.gamma = 0.99f; c0.tau = 0.01f; c0.actor_lr = c0.critic_lr = 1e-3f; c0.lambda = 10.f; c0.f1_more = f1; c0.delta = delta;
    CemPlan cp;
    auto cl = [&]() { return plan_cem_gd3pg(cem.h, s1, cem.ring_cap, c, &cp, &idx, &why); };
    c = c0; c.batch = 1; REF(cl(), INVALID, "batch 1 must be >= 2 (half of it comes from each ring)");
    c = c0; c.lambda = NAN; REF(cl(), INVALID, "gamma / tau / actor_lr / critic_lr / lambda is NaN");
    c = c0; c.delta = nullptr; REF(cl(), INVALID, "f1_more / delta is NULL (one entry per learner)");
    delta[1] = NAN; c = c0; REF(cl(), INVALID, "delta of learner 1 is NaN");
    delta[1] = 0.3f; s1[1] = 1; REF(cl(), STATE, "ring 1 (buffer_domain) of learner 1 holds 1 rows < 2: no half batch can be drawn from it");
    s1[0] = 1; REF(cl(), STATE, "ring 1 (buffer_domain) of learner 0 holds 1 rows < 2: no half batch can be drawn from it");
    s1[0] = 40; s1[1] = 40; c.batch = 18; REF(cl(), INVALID, "2 x half = 18 rows > batch_max 16");
    s1[1] = 9;      // half = 4
    int64_t ci[16] = {0, 1, 2, 39, 0, 1, 2, 39, /* learner 1 */ 0, 1, 2, 40, 0, 1, 2, 3};
    c = c0; c.idx = ci; REF(cl(), INVALID, "learner 1: idx entry 40 of ring 0 outside [0, 40) (its capacity)");
    ci[11] = -1; REF(cl(), INVALID, "learner 1: idx entry -1 of ring 0 outside [0, 40) (its capacity)");
    ci[11] = 39; ci[15] = 9; REF(cl(), INVALID, "learner 1: idx entry 9 of ring 1 outside [0, 9) (the rows it holds)");
    ci[15] = 8;
    CHECK(cl() == FRL_OK && cp.min1 == 9 && cp.half == 4 && cp.rows == 8 && cp.draw_lds == 32 && cp.ns == rowchunk_ns(cem.h, 8));
    CHECK(idx.size() == 16 && idx[3] == 39 && idx[4] == 40 && idx[7] == 79 && idx[11] == 39 && idx[15] == 48);      // ring 1's entries behind ring 0's capacity
    c.batch = 1; c.lambda = NAN; REF(cl(), INVALID, "batch 1 must be >= 2 (half of it comes from each ring)");      // the first one wins

    // ---- frl_reinforce_learn
    frl_config rc = config(FRL_ALGO_REINFORCE, {4}, {2}, 2, 256, false, 128, 64);
    rc.discrete = 1;
    const EnginePlan rf = planned(rc);
    int rs[2] = {40, 0}, ri[2] = {40, 0};
    int steps[2] = {40, 0};
    frl_reinforce_args r, r0;
    memset(&r0, 0, sizeof r0);
    r0.gamma = 0.99; r0.lr = 1e-3f; r0.n_steps = steps;
    ReinforcePlan rp;
    auto rl = [&]() { return plan_reinforce(rf.h, rs, ri, r, &rp, &why); };
    r = r0; r.gamma = NAN; REF(rl(), INVALID, "gamma / lr is NaN");
    r = r0; steps[0] = 65; REF(rl(), INVALID, "learner 0: 65 steps outside [0, capacity = 64]");
    steps[0] = -1; REF(rl(), INVALID, "learner 0: -1 steps outside [0, capacity = 64]");
    steps[0] = 40; steps[1] = 1; REF(rl(), INVALID, "learner 1 has exactly one stored step: the std of one return is NaN (the reference turns every parameter into NaN here)");
    steps[1] = 0; steps[0] = 41; REF(rl(), STATE, "learner 0: 41 steps asked for, its ring holds 40");
    steps[0] = 40; ri[0] = 3; REF(rl(), STATE, "learner 0: ring cursor (3, 40) was not filled from empty: its rows are not in time order");
    ri[0] = 40;
    CHECK(rl() == FRL_OK && rp.n_max == 40 && rp.ns == rowchunk_ns(rf.h, 40) && rp.n[0] == 40 && rp.n[1] == 0);
    r.n_steps = nullptr;      // the cursor sizes
    CHECK(rl() == FRL_OK && rp.n_max == 40 && rp.n[1] == 0);
    rs[0] = ri[0] = 0;
    CHECK(rl() == FRL_OK && rp.n_max == 0 && rp.ns == 0);      // every learner sits out: the call launches nothing
#undef REF
}

// ------------------------------------------------------------------------------------------------- plan_draw, the knob, narrow_idx
static void draws() {
    for (int b = 1; b <= 8193; ++b)
        for (int scan = 0; scan < 2; ++scan) {
            const DrawPlan d = plan_draw(b, scan != 0);
            const bool table = b >= 257 && b <= 2048 && !scan;
            CHECK(d.table == table && d.flag == (table ? 0 : 2));
            CHECK(d.lds_bytes == ((size_t)2 * ((b + 3) / 4 * 4) + (table ? 2 * 8192 : 0)) * 4);
        }
    for (int batch_max : {256, 257, 2048, 2049, 4096, 8192}) {      // (a vector reward's batch_max bounds the batch all the same: one bound)
        const size_t bound = draw_lds_max(batch_max);
        for (int b = 1; b <= batch_max; ++b) CHECK(bound >= plan_draw(b, false).lds_bytes && bound >= plan_draw(b, true).lds_bytes);
        CHECK(bound <= kDrawLdsLimit && (bound > 64 * 1024) == (batch_max >= 257));
    }
    CHECK(draw_lds_max(256) == 2048 && draw_lds_max(257) == 2 * 260 * 4 + 65536 && draw_lds_max(4096) == 81920 && kDrawLdsLimit == 81920);
    const int in[] = {0, 1, 3, 4, 6, 8, -5, 1 << 30, 0x7fffffff}, want[] = {1, 1, 2, 4, 4, 8, 1, 1 << 30, 1 << 30};
    for (int i = 0; i < 9; ++i) CHECK(clamp_stagger_groups(in[i]) == want[i]);
    CHECK(LearnKnobs().stagger_groups == 4 && LearnKnobs().stagger == 0);
    int sizes[3] = {5, 0, 7};
    const MinRing m = min_ring_size(sizes, 3, 10);
    CHECK(m.size == 0 && m.who == 1 && min_ring_size(sizes, 1, 10).size == 5 && min_ring_size(sizes, 0, 10).size == 10);
}

static int idx_mode(int argc, char** argv) {
    const std::string bound = argv[2];
    const int capacity = atoi(argv[3]), size = atoi(argv[4]);
    std::vector<int64_t> in;
    for (int i = 5; i < argc; ++i) in.push_back(atoll(argv[i]));
    std::vector<int> out;
    std::string why;
    const int n = (int)in.size();
    int rc;
    if (bound == "pair") {      // the entries as ring 1's, ring 0's all zero
        std::vector<int64_t> both(n, 0);
        both.insert(both.end(), in.begin(), in.end());
        rc = narrow_idx(IDX_RING_PAIR, both.data(), 1, 2, n, capacity, &size, &out, &why);
        for (int i = 0; rc == FRL_OK && i < n; ++i) CHECK(out[i] == 0 && out[n + i] == (int)in[i] + capacity);
    } else {
        const bool wrap = bound == "wrap";
        rc = narrow_idx(wrap ? IDX_CAPACITY_WRAP : IDX_HELD_ROWS, in.data(), 1, 1, n, capacity, &size, &out, &why);
        for (int i = 0; rc == FRL_OK && i < n; ++i) CHECK(out[i] == (int)(in[i] < 0 && wrap ? in[i] + capacity : in[i]));
    }
    if (rc != FRL_OK) { printf("refused %d: %s\n", rc, why.c_str()); return 1; }
    printf("idx ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 5 && !strcmp(argv[1], "idx")) return idx_mode(argc, argv);
    const int cases = launch_lists();
    plan_details();
    learn_refusals();
    small_refusals();
    draws();
    printf("learn_plan ok: %d launch lists\n", cases);
    return 0;
}
