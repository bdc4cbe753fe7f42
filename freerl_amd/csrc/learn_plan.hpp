// What an off-policy learn call (frl_learn, frl_envelope_learn, frl_envelope_ddpg_learn, frl_gail_learn, frl_cem_gd3pg_learn,
// frl_reinforce_learn) decides before it touches the device: which calls are refused, the arguments' defaults, how draw_kernel is
// launched, the narrowed copy of a caller's idx, and — for frl_learn — the ordered list of launches with what precedes each.  Plain
// C++17, no HIP, no getenv, so tests/learn_plan_probe.cpp states every rule on the CPU (tests/test_learn_plan.py).  The entry points
// (frl_api_learn.inc and the five frl_api_*.inc files) gather the facts, read the knobs (learn_knobs), plan, and only then flush, upload,
// take their rng_counter values and launch what the plan says.
#pragma once
#include <initializer_list>

#include "engine_plan.hpp"

namespace frl {

// The per-call developer / test knobs (read at EVERY call: the tests flip them between calls of one process).  A tri-state is -1 unset,
// 0 or 1; knob_flag() applies its default.
struct LearnKnobs {
    int dqn_fused = -1;             // FRL_DQN_FUSED (tri-state; unset: the one-launch DQN update where the shape allows it)
    int dqn_split = -1;             // FRL_DQN_SPLIT: workgroups per learner of that launch (< 0: unset)
    bool draw_scan = false;         // FRL_DRAW_SCAN=1: draw_kernel's duplicate check as a scan, no table
    bool adam_two_pass = false;     // FRL_ADAM_TWO_PASS (set at all): reduce + Adam as the two streaming launches
    int stagger = 0;                // FRL_STAGGER: sleep units between the start phases of the chained critic stage's first round
    int stagger_groups = 4;         // FRL_STAGGER_GROUPS: how many start phases; the kernel masks with it (clamp_stagger_groups)
    bool critic2_novec = false;     // FRL_CRITIC2_NOVEC (set at all): the chained critic without the aligned row loads
    bool solo_predraw = true;       // FRL_SOLO_PREDRAW=0: no spare workgroups draw the next call's rows
    bool solow_fuse = true;         // FRL_SOLOW_FUSE=0: kernels_solow.hip's policy step as two launches
};
// the largest power of two <= v, at least 1
inline int clamp_stagger_groups(int v) {
    int g = 1;
    while (g <= v / 2) g *= 2;
    return g;
}

// ---------------------------------------------------------------------------------------------- draw_kernel
// table: the duplicate check is the hash table in LDS (batches of 257 .. 2048 rows; device/net.hpp), else the scan; lds_bytes: the two
// index arrays [+ the table's two halves]; flag: what the kernel takes in bit 1 of want_noise
struct DrawPlan { bool table; size_t lds_bytes; int flag; };
inline DrawPlan plan_draw(int batch, bool scan) {
    DrawPlan d;
    d.table = batch > 256 && 4 * batch <= kDrawTableHost && !scan;
    d.lds_bytes = ((size_t)2 * ((batch + 3) & ~3) + (d.table ? 2 * kDrawTableHost : 0)) * sizeof(int);
    d.flag = d.table ? 0 : 2;
    return d;
}
// the most a draw may ask for: 2048 rows with the table (what a device draw past it is refused against)
constexpr size_t kDrawLdsLimit = (size_t)(2 * 2048 + 2 * kDrawTableHost) * sizeof(int);
// the most any batch of 1 .. draw_rows_max asks for (both regimes grow with the batch): frl_create's hipFuncAttributeMaxDynamicSharedMemorySize
inline size_t draw_lds_max(int draw_rows_max) {
    return std::min(kDrawLdsLimit, std::max(plan_draw(draw_rows_max, false).lds_bytes, plan_draw(std::min(draw_rows_max, kDrawTableHost / 4), false).lds_bytes));
}
inline int refuse_draw(int batch, std::string* message) {
    return plan_refuse(message, "device index draw of %d rows does not fit the draw kernel's LDS; pass idx", batch);
}

// ---------------------------------------------------------------------------------------------- shared pieces
// a refusal with FRL_ERR_STATE (plan_refuse's own code is FRL_ERR_INVALID)
#define FRL_REFUSE_STATE(...) (plan_refuse(__VA_ARGS__), FRL_ERR_STATE)

// the smallest ring of the population and the first learner that holds it (sizes never exceed the capacity)
struct MinRing { int size, who; };
inline MinRing min_ring_size(const int* sizes, int P, int capacity) {
    MinRing m{capacity, 0};
    for (int p = 0; p < P; ++p)
        if (sizes[p] < m.size) m = {sizes[p], p};
    return m;
}

inline int refuse_nan(std::initializer_list<float> scalars, const char* names, std::string* message) {
    for (const float v : scalars)
        if (!(v == v)) return plan_refuse(message, "%s is NaN", names);
    return FRL_OK;
}

// A caller's int64 rows [P][sets][n], range-checked and narrowed into *out (same shape).  The three bounds in use:
// IDX_CAPACITY_WRAP (frl_learn, the envelope calls): [-capacity, capacity), negative entries count from the end;
// IDX_HELD_ROWS (frl_gail_learn): [0, sizes[p]); IDX_RING_PAIR (frl_cem_gd3pg_learn, sets = 2): ring 0 below its capacity — rows never
// written are zeros, as the reference's — ring 1 below sizes[p] (ring 1's sizes), its entries moved up by `capacity`
enum IdxBound { IDX_CAPACITY_WRAP, IDX_HELD_ROWS, IDX_RING_PAIR };
inline int narrow_idx(IdxBound bound, const int64_t* idx, int P, int sets, int n, int capacity, const int* sizes, std::vector<int>* out, std::string* message) {
    out->resize((size_t)P * sets * n);
    for (int p = 0; p < P; ++p)
        for (int s = 0; s < sets; ++s) {
            const int64_t* src = idx + ((size_t)p * sets + s) * n;
            int* dst = out->data() + ((size_t)p * sets + s) * n;
            for (int i = 0; i < n; ++i) {
                int64_t v = src[i];
                if (bound == IDX_CAPACITY_WRAP) {
                    if (v < 0) v += capacity;
                    if (v < 0 || v >= capacity) return plan_refuse(message, "sample index %lld out of range", (long long)src[i]);
                } else if (bound == IDX_HELD_ROWS) {
                    if (v < 0 || v >= sizes[p])
                        return FRL_REFUSE_STATE(message, "idx entry %lld of learner %d is not one of its %d stored rows", (long long)v, p, sizes[p]);
                } else {
                    const int lim = s == 0 ? capacity : sizes[p];
                    if (v < 0 || v >= lim)
                        return plan_refuse(message, "learner %d: idx entry %lld of ring %d outside [0, %d) (%s)", p, (long long)v, s, lim,
                                           s == 0 ? "its capacity" : "the rows it holds");
                    v += (int64_t)s * capacity;
                }
                dst[i] = (int)v;
            }
        }
    return FRL_OK;
}

// ---------------------------------------------------------------------------------------------- frl_learn
// What plan_learn needs from the engine next to its descriptor.  min_size: the smallest ring — for a pre-armed rollout launch the size
// WHEN THE LAUNCH RUNS; predraw_bufs: the pre-draw slots exist (d_solo_pre); ma_pre_*: what the last multi-agent kernels_solow.hip critic
// launch's spare workgroups drew for; rng_counter: the value this call would take
struct LearnFacts {
    const EngineDesc* h = nullptr;
    const EngineFacts* f = nullptr;
    int min_size = 0;
    bool per_on = false, predraw_bufs = false;
    bool ma_pre_valid = false;
    unsigned long long ma_pre_counter = 0;
    int ma_pre_size = 0, ma_pre_batch = 0;
    unsigned long long rng_counter = 0;
};
// what frl_rollout folds into the step (FOLD_NONE: a plain frl_learn)
enum LearnFold { LEARN_PLAIN, LEARN_FOLD_DQN, LEARN_FOLD_SOLO };

// One launch_learn_stage: stage 0 critic | Q, 1 actor (agent: MASAC's and MAAC's one agent per launch), 2 the soft update; units = (learner, agent)
// pairs.  draw / obsnorm / noisy_materialise: draw_kernel, obsnorm_kernel, noisy_materialise_kernel run in front of it
struct LearnLaunch { int stage = 0, agent = 0, units = 0; bool draw = false, obsnorm = false, noisy_materialise = false; };
struct LearnPlan {
    LearnArgs a;
    LearnFamily fam = FAM_ROWCHUNK;
    bool dev_rng = false, needs_noise = false;
    // NoisyLinear heads: the first of the three noise sets a call uses (the reference draws per forward in program order: [online(s') if
    // Double,] target(s'), online(s)); device_draw: noisy_draw_kernel fills them with the NEXT rng_counter value, else the caller's are uploaded
    bool noisy = false, noisy_device_draw = false;
    int noisy_first = 0;
    int counters = 1;               // rng_counter values the call takes
    DrawPlan draw{false, 0, 2};
    bool critic_nv = false;         // the chained critic with aligned next_obs / (reward, done) loads
    // kernels_solo.hip / kernels_solow.hip: the critic launch reads a pre-drawn slot / may have spare workgroups write the next call's;
    // pre_multi: the multi-agent slots (one spare workgroup per unit when it writes), else one per learner on kernels_solo.hip, the
    // learners' own helpers on single-agent kernels_solow.hip (touch: the slots' sequence advances at all)
    bool pre_touch = false, pre_read = false, pre_write = false, pre_multi = false;
    int pre_extra = 0;
    int head[2] = {0, 0}, tail[2] = {0, 0};      // a folded solo step: SoloStepArgs::head / tail of the critic and the actor launch
    int n_launches = 0;
    LearnLaunch launches[2 * FRL_MAX_AGENTS + 2];      // (the most: MAAC's critic and actor launch per agent, then the soft stage)
};

// FRL_OK and *out, or the refusal's code and *message: everything that can refuse a frl_learn, in one order, before anything is flushed,
// uploaded or counted.  idx_out: a caller's idx narrowed (untouched when args.idx is NULL).
inline int plan_learn(const LearnFacts& F, const LearnKnobs& k, const frl_learn_args& args, LearnFold fold, LearnPlan* out, std::vector<int>* idx_out,
                      std::string* message) {
    const EngineDesc& h = *F.h;
    const EngineFacts& f = *F.f;
    const int B = args.batch, min_size = F.min_size;
    if (B < 1 || B > h.batch_max) return plan_refuse(message, "batch %d outside [1,%d]", B, h.batch_max);
    if (min_size < B) return FRL_REFUSE_STATE(message, "a ring holds %d rows < batch %d", min_size, B);
    if (args.per && (h.algo != FRL_ALGO_DQN || !F.per_on)) return FRL_REFUSE_STATE(message, "per = 1 needs a DQN engine with frl_per_enable");
    if (args.per && args.idx) return plan_refuse(message, "per = 1 uses the rows of the last frl_per_sample; idx must be NULL");
    LearnPlan pl;
    pl.dev_rng = args.idx == nullptr && !args.per;
    if (pl.dev_rng && min_size < 2 * B) return FRL_REFUSE_STATE(message, "device index draw needs len(buffer) >= 2*batch (have %d); pass idx", min_size);
    const bool maddpg = is_maddpg(h.algo), masac = h.algo == FRL_ALGO_MASAC, maac = h.algo == FRL_ALGO_MAAC, dqn = h.algo == FRL_ALGO_DQN;
    const bool td3_like = h.algo == FRL_ALGO_TD3 || maddpg;            // MADDPG + noise/delay = MATD3_simple.py (ATT-MADDPG: do_actor only)
    pl.needs_noise = h.algo == FRL_ALGO_SAC || masac || maac || (td3_like && args.use_policy_noise);      // (MAAC: Exp(1) draws, not normal ones)
    if (masac && args.use_policy_noise) return FRL_REFUSE_STATE(message, "frl_learn: MASAC has no target policy smoothing (MATD3's): use_policy_noise must be 0");
    if (masac && args.loss_kind == FRL_LOSS_HUBER) return plan_refuse(message, "MASAC's critic loss is F.mse_loss (MASAC.py:241): no Huber variant");
    if (maac && args.use_policy_noise) return FRL_REFUSE_STATE(message, "frl_learn: MAAC has no target policy smoothing (MATD3's): use_policy_noise must be 0");
    if (maac && args.loss_kind == FRL_LOSS_HUBER) return plan_refuse(message, "MAAC's critic loss is MSELoss (MAAC_discrete.py:236): no Huber variant");
    if (h.algo == FRL_ALGO_MADDPG_ATT && args.use_policy_noise) return plan_refuse(message, "ATT-MADDPG has no target policy smoothing: use_policy_noise must be 0");
    if (!pl.dev_rng && pl.needs_noise && !args.noise) return plan_refuse(message, "idx given without noise: both or neither");
    if (args.idx)
        if (const int rc = narrow_idx(IDX_CAPACITY_WRAP, args.idx, h.P, h.n_agents, B, h.capacity, nullptr, idx_out, message)) return rc;
    if (args.loss_kind != FRL_LOSS_MSE && args.loss_kind != FRL_LOSS_HUBER) return plan_refuse(message, "unknown loss_kind %d", args.loss_kind);
    if (args.loss_kind == FRL_LOSS_HUBER) {
        if (!(args.huber_delta > 0.f)) return plan_refuse(message, "Huber loss needs huber_delta > 0");
        if (h.c51_atoms) return FRL_REFUSE_STATE(message, "the Categorical head's loss is a cross-entropy: no Huber variant");
        if (h.algo == FRL_ALGO_SAC_DISCRETE) return plan_refuse(message, "discrete SAC's critic loss is F.mse_loss (SAC_add_discrete.py:313-314): no Huber variant");
    }
    pl.fam = learn_family(h, f.family, B, knob_flag(k.dqn_fused, true));
    if (fold == LEARN_FOLD_SOLO && (pl.fam != FAM_SOLO || !pl.dev_rng)) return FRL_REFUSE_STATE(message, "step fusion needs a solo engine with device draws");
    // who draws: kernels_solo.hip, single-agent kernels_solow.hip and the one-launch DQN update in their critic launch, else draw_kernel —
    // unless the previous multi-agent kernels_solow.hip launch drew for exactly this counter, ring size and batch (MADDPG without smoothing noise)
    const LearnFamily fam = pl.fam;
    const bool draws_in_critic = fam == FAM_DQN_FUSED || fam == FAM_SOLO || (fam == FAM_SOLOW && h.n_agents == 1);
    const bool ma_predraw = fam == FAM_SOLOW && h.n_agents > 1 && pl.dev_rng && !pl.needs_noise;
    const bool ma_use_pre = ma_predraw && F.ma_pre_valid && F.ma_pre_counter == F.rng_counter && F.ma_pre_size == min_size && F.ma_pre_batch == B;
    const bool draw_kernel_runs = pl.dev_rng && !draws_in_critic && !ma_use_pre;
    pl.draw = plan_draw(B, k.draw_scan);
    if (draw_kernel_runs && pl.draw.lds_bytes > kDrawLdsLimit) return refuse_draw(B, message);

    LearnArgs& a = pl.a;
    memset(&a, 0, sizeof a);
    a.batch = B;
    a.size = min_size;
    a.device_rng = pl.dev_rng ? 1 : 0;
    a.do_actor = td3_like ? (args.do_actor ? 1 : 0) : 1;
    a.gamma = args.gamma; a.tau = args.tau;
    a.actor_lr = args.actor_lr; a.critic_lr = args.critic_lr; a.alpha_lr = args.alpha_lr;
    a.adam_eps = args.adam_eps > 0 ? args.adam_eps : 1e-8f;
    a.beta1 = 0.9f; a.beta2 = 0.999f;
    a.critic_wd = args.critic_weight_decay;
    a.clip_norm = args.clip_norm;
    a.policy_noise = args.policy_noise; a.noise_clip = args.noise_clip;
    a.max_action = args.max_action != 0.f ? args.max_action : 1.f;
    a.policy_noise_scale = args.policy_noise_scale;
    a.use_policy_noise = (td3_like && args.use_policy_noise) ? 1 : 0;
    a.target_entropy = args.target_entropy;
    a.double_dqn = (dqn && args.double_dqn) ? 1 : 0;
    a.use_isw = (dqn && args.per) ? (args.per == 2 ? 2 : 1) : 0;
    if (args.loss_kind == FRL_LOSS_HUBER) { a.huber = 1; a.huber_delta = args.huber_delta; }
    a.rng_counter = F.rng_counter;
    a.p0 = 0; a.p_count = h.P;
    if (h.noisy) {
        pl.noisy = true;
        pl.noisy_first = a.double_dqn ? 0 : 1;
        pl.noisy_device_draw = args.noisy_eps == nullptr;
        if (pl.noisy_device_draw) pl.counters = 2;
    }
    if (fam == FAM_DQN_FUSED) a.dqn_split = dqn_split_for(h, B, h.P, k.dqn_split);
    if (fam == FAM_CHAINED) {
        // (developer knob: spread the Adam bursts of the first round)
        a.stagger = k.stagger; a.stagger_groups = k.stagger_groups; a.stagger_wgs = f.n_cus;
        // (_nv: next_obs 16-byte aligned with its 16 columns inside the row, (reward, done) an aligned pair)
        const RecordDesc& R = h.rec;
        pl.critic_nv = R.nobs_off[0] % 4 == 0 && R.nobs_off[0] + 16 <= R.stride && R.rew_off % 2 == 0 && R.done_off == R.rew_off + 1 && !k.critic2_novec;
    }
    // (kernels_solow.hip moves MADDPG's targets at the end of its actor launch)
    const bool actor_stage = !dqn && a.do_actor, soft_stage = maddpg && a.do_actor && fam != FAM_SOLOW;
    // kernels_solow.hip, single agent, helper workgroups present: a policy step is ONE launch — the critic's update runs on the helpers
    // under the policy's forward (FRL_SOLOW_FUSE=0: two launches)
    if (actor_stage && fam == FAM_SOLOW && h.n_agents == 1 && f.solow_wgs > f.solow_row_wgs) a.fuse_actor = k.solow_fuse ? 1 : 0;
    // the next call's rows drawn by spare workgroups of this critic launch, which need a CU of their own next to the learners'
    const int units = h.P * h.n_agents;
    if (fam == FAM_SOLO && pl.dev_rng && fold == LEARN_PLAIN && F.predraw_bufs) {
        pl.pre_touch = pl.pre_read = true;
        pl.pre_write = h.P * (h.solo + 1) <= f.n_cus && k.solo_predraw;
        pl.pre_extra = pl.pre_write ? h.P : 0;
    } else if (fam == FAM_SOLOW && h.n_agents == 1 && pl.dev_rng && F.predraw_bufs) {      // the learners' first helper workgroups draw
        pl.pre_touch = pl.pre_read = true;
        pl.pre_write = f.solow_wgs > f.solow_row_wgs && k.solo_predraw;
    } else if (fam == FAM_SOLOW && h.n_agents > 1) {      // one spare workgroup per unit draws, the duplicate table in its own LDS
        pl.pre_touch = pl.pre_multi = true;
        pl.pre_read = ma_use_pre;
        pl.pre_write = ma_predraw && units * (f.solow_wgs + 1) <= f.n_cus && k.solo_predraw;
        pl.pre_extra = pl.pre_write ? units : 0;
    }
    // frl_rollout on a solo engine: the step's add() rides at the head of the critic launch, its tail (obs advance + the next select_action
    // + hand-over) at the end of the step's LAST launch
    if (fold == LEARN_FOLD_SOLO) { pl.head[0] = 1; pl.tail[0] = actor_stage ? 0 : 1; pl.head[1] = 0; pl.tail[1] = 1; }

    auto push = [&](int stage, int agent) -> LearnLaunch& {
        LearnLaunch& l = pl.launches[pl.n_launches++];
        l.stage = stage; l.agent = agent; l.units = units;
        return l;
    };
    if (fam == FAM_MAAC) {      // DESIGN.md "MAAC": per agent, in agent order, critic i (+ its reduce and step) then actor i (+ its); then every target
        for (int ag = 0; ag < h.n_agents; ++ag) {
            push(0, ag).draw = ag == 0 && draw_kernel_runs;
            push(1, ag);
        }
        push(2, 0);
        *out = pl;
        return FRL_OK;
    }
    LearnLaunch& c = push(0, 0);
    if (fam != FAM_DQN_FUSED) {      // (the one-launch DQN update draws, normalises and materialises for itself)
        c.draw = draw_kernel_runs;
        c.obsnorm = h.obs_norm_on && !dqn;      // sample(): norm(obs) updates the statistics first
        c.noisy_materialise = h.noisy != 0;
    }
    if (fam == FAM_MASAC) {      // DESIGN.md "MASAC": behind all the critics the agents' actor + alpha steps one after the other, then every target
        for (int ag = 0; ag < h.n_agents; ++ag) push(1, ag);
    } else if (actor_stage && !a.fuse_actor) {
        push(1, 0);
    }
    if (soft_stage || fam == FAM_MASAC) push(2, 0);
    *out = pl;
    return FRL_OK;
}

// ---------------------------------------------------------------------------------------------- the envelope calls
// Both envelope entry points: rows = batch x weight_num, ns = slabs per learner of the gradient launch
struct EnvelopeCall {
    int batch, weight_num;
    float gamma, beta;
    const int64_t* idx;
    const float* weights;
};
struct EnvelopePlan { int rows = 0, ns = 0, min_size = 0; bool dev_idx = false; DrawPlan draw{false, 0, 2}; };
inline int plan_envelope(const EngineDesc& h, const int* sizes, const EnvelopeCall& c, std::initializer_list<float> scalars, const char* scalar_names,
                         EnvelopePlan* out, std::vector<int>* idx_out, std::string* message) {
    const int B = c.batch, W = c.weight_num;
    if (B < 1) return plan_refuse(message, "batch %d must be >= 1", B);
    if (W < 1) return plan_refuse(message, "weight_num %d must be >= 1", W);
    if ((long long)B * W > h.batch_max) return plan_refuse(message, "batch %d x weight_num %d = %lld rows > batch_max %d", B, W, (long long)B * W, h.batch_max);
    if (const int rc = refuse_nan(scalars, scalar_names, message)) return rc;
    if (c.beta < 0.f || c.beta > 1.f) return plan_refuse(message, "beta %g outside [0, 1]", (double)c.beta);
    EnvelopePlan pl;
    pl.min_size = min_ring_size(sizes, h.P, h.capacity).size;
    if (pl.min_size < B) return FRL_REFUSE_STATE(message, "a ring holds %d rows < batch %d", pl.min_size, B);
    pl.dev_idx = c.idx == nullptr;
    pl.draw = plan_draw(B, false);
    if (pl.dev_idx && pl.min_size < 2 * B) return FRL_REFUSE_STATE(message, "device index draw needs len(buffer) >= 2*batch (have %d); pass idx", pl.min_size);
    if (pl.dev_idx && pl.draw.lds_bytes > kDrawLdsLimit) return refuse_draw(B, message);
    if (c.idx)
        if (const int rc = narrow_idx(IDX_CAPACITY_WRAP, c.idx, h.P, 1, B, h.capacity, nullptr, idx_out, message)) return rc;
    pl.rows = B * W;
    pl.ns = rowchunk_ns(h, pl.rows);
    *out = pl;
    return FRL_OK;
}

// ---------------------------------------------------------------------------------------------- frl_gail_learn
struct GailPlan { int min_size = 0, ns = 0; };
inline int plan_gail(const EngineDesc& h, const int* sizes, const frl_gail_args& args, GailPlan* out, std::vector<int>* idx_out, std::string* message) {
    const int E = args.n_expert, NP = args.n_policy;
    if (E < 1 || E > h.batch_max) return plan_refuse(message, "n_expert %d outside [1, batch_max %d]", E, h.batch_max);
    if (NP < 1 || NP > h.batch_max) return plan_refuse(message, "n_policy %d outside [1, batch_max %d]", NP, h.batch_max);
    if (args.gp != 0 && args.gp != 1) return plan_refuse(message, "gp %d must be 0 or 1", args.gp);
    if (const int rc = refuse_nan({args.gp_weight, args.lr, args.beta1, args.beta2, args.adam_eps}, "gp_weight / lr / beta1 / beta2 / adam_eps", message)) return rc;
    if (args.gp_weight < 0.f) return plan_refuse(message, "gp_weight %g must be >= 0", (double)args.gp_weight);
    if (args.beta1 < 0.f || args.beta1 >= 1.f || args.beta2 < 0.f || args.beta2 >= 1.f)
        return plan_refuse(message, "betas (%g, %g) outside [0, 1)", (double)args.beta1, (double)args.beta2);
    if (!args.policy_rows) return plan_refuse(message, "policy_rows is NULL");
    GailPlan pl;
    pl.min_size = min_ring_size(sizes, h.P, h.capacity).size;
    if (pl.min_size < 1) return FRL_REFUSE_STATE(message, "a learner's ring is empty: store the expert rows first");
    if (args.idx)
        if (const int rc = narrow_idx(IDX_HELD_ROWS, args.idx, h.P, 1, E, h.capacity, sizes, idx_out, message)) return rc;
    pl.ns = rowchunk_ns(h, E + NP);
    *out = pl;
    return FRL_OK;
}

// ---------------------------------------------------------------------------------------------- frl_cem_gd3pg_learn
// sample() (CEM_GD3PG.py:160-164): total = len(buffer_domain) bounds the batch AND both draws; the population shares one launch shape, so
// its smallest ring 1 decides.  size1: ring 1's sizes; ring_cap: rows of one ring
struct CemPlan { int min1 = 0, half = 0, rows = 0, ns = 0; size_t draw_lds = 0; };
inline int plan_cem_gd3pg(const EngineDesc& h, const int* size1, int ring_cap, const frl_cem_gd3pg_args& args, CemPlan* out, std::vector<int>* idx_out,
                          std::string* message) {
    if (args.batch < 2) return plan_refuse(message, "batch %d must be >= 2 (half of it comes from each ring)", args.batch);
    if (const int rc = refuse_nan({args.gamma, args.tau, args.actor_lr, args.critic_lr, args.lambda}, "gamma / tau / actor_lr / critic_lr / lambda", message)) return rc;
    if (!args.f1_more || !args.delta) return plan_refuse(message, "f1_more / delta is NULL (one entry per learner)");
    for (int p = 0; p < h.P; ++p)
        if (!(args.delta[p] == args.delta[p])) return plan_refuse(message, "delta of learner %d is NaN", p);
    const MinRing m = min_ring_size(size1, h.P, ring_cap);
    if (m.size < 2) return FRL_REFUSE_STATE(message, "ring 1 (buffer_domain) of learner %d holds %d rows < 2: no half batch can be drawn from it", m.who, m.size);
    CemPlan pl;
    pl.min1 = m.size;
    pl.half = std::min(m.size, args.batch) / 2;
    pl.rows = 2 * pl.half;
    if (pl.rows > h.batch_max) return plan_refuse(message, "2 x half = %d rows > batch_max %d", pl.rows, h.batch_max);
    pl.draw_lds = (size_t)2 * ((pl.half + 3) & ~3) * sizeof(int);
    if (!args.idx && pl.draw_lds > 64 * 1024) return plan_refuse(message, "device index draw of 2 x %d rows does not fit the draw kernel's LDS; pass idx", pl.half);
    if (args.idx)
        if (const int rc = narrow_idx(IDX_RING_PAIR, args.idx, h.P, 2, pl.half, ring_cap, size1, idx_out, message)) return rc;
    pl.ns = rowchunk_ns(h, pl.rows);
    *out = pl;
    return FRL_OK;
}

// ---------------------------------------------------------------------------------------------- frl_popart_ddpg_learn
// sample() (DDPG_simple_with_tricks.py:244-250): rows = min(len(buffer), batch_size); the population shares one launch shape, so its
// smallest ring decides.  The device draw is draw_kernel's, with its rule (a ring of at least 2 x rows rows)
struct PopartPlan { int min_size = 0, rows = 0, ns = 0; bool dev_idx = false; DrawPlan draw{false, 0, 2}; };
inline int plan_popart_ddpg(const EngineDesc& h, const int* sizes, const frl_popart_ddpg_args& args, PopartPlan* out, std::vector<int>* idx_out,
                            std::string* message) {
    if (args.batch < 1) return plan_refuse(message, "batch %d must be >= 1", args.batch);
    if (const int rc = refuse_nan({args.gamma, args.tau, args.actor_lr, args.critic_lr, args.upper_lr, args.beta},
                                  "gamma / tau / actor_lr / critic_lr / upper_lr / beta", message)) return rc;
    if (args.beta < 0.f || args.beta > 1.f) return plan_refuse(message, "beta %g outside [0, 1]", (double)args.beta);
    const MinRing m = min_ring_size(sizes, h.P, h.capacity);
    if (m.size < 1) return FRL_REFUSE_STATE(message, "the ring of learner %d is empty: no batch can be drawn from it", m.who);
    PopartPlan pl;
    pl.min_size = m.size;
    pl.rows = std::min(m.size, args.batch);
    if (pl.rows > h.batch_max) return plan_refuse(message, "min(len(buffer), batch) = %d rows > batch_max %d", pl.rows, h.batch_max);
    pl.dev_idx = args.idx == nullptr;
    pl.draw = plan_draw(pl.rows, false);
    if (pl.dev_idx && m.size < 2 * pl.rows) return FRL_REFUSE_STATE(message, "device index draw needs len(buffer) >= 2*batch (have %d); pass idx", m.size);
    if (pl.dev_idx && pl.draw.lds_bytes > kDrawLdsLimit) return refuse_draw(pl.rows, message);
    if (args.idx)
        if (const int rc = narrow_idx(IDX_CAPACITY_WRAP, args.idx, h.P, 1, pl.rows, h.capacity, nullptr, idx_out, message)) return rc;
    pl.ns = rowchunk_ns(h, pl.rows);
    *out = pl;
    return FRL_OK;
}

// ---------------------------------------------------------------------------------------------- frl_reinforce_learn
// n[p]: the rows learner p trains on (0: it sits the call out); n_max == 0: every learner sits out and the call launches nothing
struct ReinforcePlan { int n_max = 0, ns = 0; std::vector<int> n; };
inline int plan_reinforce(const EngineDesc& h, const int* sizes, const int* index, const frl_reinforce_args& args, ReinforcePlan* out, std::string* message) {
    if (!(args.gamma == args.gamma) || !(args.lr == args.lr)) return plan_refuse(message, "%s is NaN", "gamma / lr");      // (doubles: not refuse_nan's floats)
    out->n.resize(h.P);
    out->n_max = 0;
    for (int p = 0; p < h.P; ++p) {
        const int n = args.n_steps ? args.n_steps[p] : sizes[p];
        if (n < 0 || n > h.capacity) return plan_refuse(message, "learner %d: %d steps outside [0, capacity = %d]", p, n, h.capacity);
        if (n == 1)
            return plan_refuse(message, "learner %d has exactly one stored step: the std of one return is NaN "
                                        "(the reference turns every parameter into NaN here)", p);
        if (n > sizes[p]) return FRL_REFUSE_STATE(message, "learner %d: %d steps asked for, its ring holds %d", p, n, sizes[p]);
        if (n > 0 && index[p] != sizes[p] % h.capacity)      // rows 0..n-1 are in time order only in a ring filled from an empty cursor
            return FRL_REFUSE_STATE(message, "learner %d: ring cursor (%d, %d) was not filled from empty: its rows are not in time order", p, index[p], sizes[p]);
        out->n[p] = n;
        out->n_max = std::max(out->n_max, n);
    }
    out->ns = out->n_max ? rowchunk_ns(h, out->n_max) : 0;      // workgroups (= slabs) of the longest episode
    return FRL_OK;
}

}  // namespace frl
