// frl_learn(): the ONE table of the kernel families' kernels and LDS bytes (a new family is registered there; which family an engine
// learns with is engine_plan.hpp's decision), a launcher per family, learn_impl and the work models.  Part of frl_api.hip.

// --------------------------------------------------------------------------- the family table
enum LearnKernelStage { LK_CRITIC, LK_CRITIC_NV, LK_ACTOR, LK_ACTOR_RECOMPUTE, LK_STEP };
struct LearnKernelRow {
    LearnFamily fam;
    int stage;          // LK_CRITIC_NV: the 8-wave chained critic with aligned next_obs / (reward, done) loads; LK_STEP: a whole policy step;
                        // LK_ACTOR_RECOMPUTE: the 8-wave chained actor stage without the park buffer (FRL_ACTOR_PARK=0)
    int sub;            // FAM_CHAINED: waves per workgroup; FAM_SOLO: workgroups per learner; FAM_SOLOW: 1 single-agent, 2 (learner, agent) units
    int lds_bytes;      // dynamic LDS of the launch = the kernels' hipFuncAttributeMaxDynamicSharedMemorySize (engine_plan.hpp: family_lds_bytes)
    KernelPtr k[2][2];  // [critic heads - 1][16-column tiles of the actor head - 1]
};
static const LearnKernelRow kLearnKernels[] = {
    {FAM_DQN_FUSED, LK_CRITIC, 0, kLdsDqnFused, {{dqn_fused_kernel, dqn_fused_kernel}, {dqn_fused_kernel, dqn_fused_kernel}}},
    // the register-chained family: one workgroup per learner with the nets as LDS images (156 KB)
    {FAM_CHAINED, LK_CRITIC, 8, kLdsChain8, {{ac_critic_v2_single_kernel, ac_critic_v2_single_kernel}, {ac_critic_v2_twin_kernel, ac_critic_v2_twin_kernel}}},
    {FAM_CHAINED, LK_CRITIC_NV, 8, kLdsChain8, {{ac_critic_v2_single_nv_kernel, ac_critic_v2_single_nv_kernel}, {ac_critic_v2_twin_nv_kernel, ac_critic_v2_twin_nv_kernel}}},
    {FAM_CHAINED, LK_ACTOR, 8, kLdsChain8, {{ac_actor_v2_kernel, ac_actor_v2_kernel}, {ac_actor_v2_kernel, ac_actor_v2_kernel}}},
    {FAM_CHAINED, LK_ACTOR_RECOMPUTE, 8, kLdsChain8, {{ac_actor_v2_recompute_kernel, ac_actor_v2_recompute_kernel}, {ac_actor_v2_recompute_kernel, ac_actor_v2_recompute_kernel}}},
    {FAM_CHAINED, LK_CRITIC, 4, kLdsChain4, {{ac_critic_v2w4_single_kernel, ac_critic_v2w4_single_kernel}, {ac_critic_v2w4_twin_kernel, ac_critic_v2w4_twin_kernel}}},
    {FAM_CHAINED, LK_ACTOR, 4, kLdsChain4, {{ac_actor_v2w4_kernel, ac_actor_v2w4_kernel}, {ac_actor_v2w4_kernel, ac_actor_v2w4_kernel}}},
    {FAM_SOLO, LK_CRITIC, 16, kLdsSolo, {{solo_critic_single_kernel, solo_critic_single_kernel}, {solo_critic_twin_kernel, solo_critic_twin_kernel}}},
    {FAM_SOLO, LK_ACTOR, 16, kLdsSolo, {{solo_actor_kernel, solo_actor_kernel}, {solo_actor_kernel, solo_actor_kernel}}},
    {FAM_SOLO, LK_CRITIC, 8, kLdsSolo, {{solo_critic_single_w8_kernel, solo_critic_single_w8_kernel}, {solo_critic_twin_w8_kernel, solo_critic_twin_w8_kernel}}},
    {FAM_SOLO, LK_ACTOR, 8, kLdsSolo, {{solo_actor_w8_kernel, solo_actor_w8_kernel}, {solo_actor_w8_kernel, solo_actor_w8_kernel}}},
    {FAM_SOLOW, LK_CRITIC, 1, kLdsSolow, {{solow_critic_h1a1_kernel, solow_critic_h1a2_kernel}, {solow_critic_h2a1_kernel, solow_critic_h2a2_kernel}}},
    {FAM_SOLOW, LK_ACTOR, 1, kLdsSolow, {{solow_actor_a1_kernel, solow_actor_a2_kernel}, {solow_actor_a1_kernel, solow_actor_a2_kernel}}},
    {FAM_SOLOW, LK_STEP, 1, kLdsSolow, {{solow_step_h1a1_kernel, solow_step_h1a2_kernel}, {solow_step_h2a1_kernel, solow_step_h2a2_kernel}}},
    {FAM_SOLOW, LK_CRITIC, 2, kLdsSolow, {{solow_critic_ma_h1a1_kernel, solow_critic_ma_h1a2_kernel}, {solow_critic_ma_h2a1_kernel, solow_critic_ma_h2a2_kernel}}},
    {FAM_SOLOW, LK_ACTOR, 2, kLdsSolow, {{solow_actor_ma_a1_kernel, solow_actor_ma_a2_kernel}, {solow_actor_ma_a1_kernel, solow_actor_ma_a2_kernel}}},
    {FAM_WIDE, LK_CRITIC, 0, kLdsWide, {{ac_critic_wide_h1a1_kernel, ac_critic_wide_h1a2_kernel}, {ac_critic_wide_h2a1_kernel, ac_critic_wide_h2a2_kernel}}},
    {FAM_WIDE, LK_ACTOR, 0, kLdsWide, {{ac_actor_wide_a1_kernel, ac_actor_wide_a2_kernel}, {ac_actor_wide_a1_kernel, ac_actor_wide_a2_kernel}}},
    {FAM_WIDE16, LK_CRITIC, 0, kLdsWide16, {{ac_critic_x_h1a1_kernel, ac_critic_x_h1a2_kernel}, {ac_critic_x_h2a1_kernel, ac_critic_x_h2a2_kernel}}},
    {FAM_WIDE16, LK_ACTOR, 0, kLdsWide16, {{ac_actor_x_a1_kernel, ac_actor_x_a2_kernel}, {ac_actor_x_a1_kernel, ac_actor_x_a2_kernel}}},
    // the attention critic of ATT-MADDPG on the row-chunk skeleton (kernels_att.hip): kLdsAtt is the launches' limit, a launch carves the engine's own bytes
    {FAM_ATT, LK_CRITIC, 0, kLdsAtt, {{att_critic_kernel, att_critic_kernel}, {att_critic_kernel, att_critic_kernel}}},
    {FAM_ATT, LK_ACTOR, 0, kLdsAtt, {{att_actor_kernel, att_actor_kernel}, {att_actor_kernel, att_actor_kernel}}},
    // MASAC on the row-chunk skeleton (kernels_masac.hip): the critic launch over (learner, agent) units, the actor launch over learners for one agent
    {FAM_MASAC, LK_CRITIC, 0, kLdsMasac, {{masac_critic_kernel, masac_critic_kernel}, {masac_critic_kernel, masac_critic_kernel}}},
    {FAM_MASAC, LK_ACTOR, 0, kLdsMasac, {{masac_actor_kernel, masac_actor_kernel}, {masac_actor_kernel, masac_actor_kernel}}},
};

// every kernel of the family may carve its row's LDS bytes, whichever of them the engine's shape resolves to
static hipError_t set_family_lds_attributes(LearnFamily fam) {
    for (const LearnKernelRow& r : kLearnKernels)
        for (int i = 0; i < 4 && r.fam == fam; ++i) {
            const hipError_t err = hipFuncSetAttribute(r.k[i / 2][i % 2].address(), hipFuncAttributeMaxDynamicSharedMemorySize, r.lds_bytes);
            if (err != hipSuccess) return err;
        }
    return hipSuccess;
}

// the kernels `fam` runs on this engine: the twin / head-tile / waves / workgroups / multi-agent selections, made once at frl_create
// actor_park: the engine's FRL_ACTOR_PARK (EngineFacts); false picks the family's LK_ACTOR_RECOMPUTE kernel where it has one (eight waves)
static LearnKernels resolve_learn_kernels(LearnFamily fam, int chain_waves, bool actor_park, const EngineDesc& h) {
    const int twin = h.net[1].heads == 2, a2 = h.net[0].L[2].n_pad > 16;
    const int sub = fam == FAM_CHAINED ? chain_waves : fam == FAM_SOLO ? h.solo : fam == FAM_SOLOW ? (h.n_agents > 1 ? 2 : 1) : 0;
    LearnKernels K;
    KernelPtr recompute;
    K.block = (fam == FAM_CHAINED && sub == 8) ? 512 : 256;
    for (const LearnKernelRow& r : kLearnKernels) {
        if (r.fam != fam || r.sub != sub) continue;
        K.lds_bytes = r.lds_bytes;
        if (r.stage == LK_ACTOR_RECOMPUTE) { recompute = r.k[twin][a2]; continue; }
        (r.stage == LK_CRITIC ? K.critic : r.stage == LK_CRITIC_NV ? K.critic_nv : r.stage == LK_ACTOR ? K.actor : K.step) = r.k[twin][a2];
    }
    if (!actor_park && recompute.k) K.actor = recompute;
    return K;
}

// The family THIS call runs and the workgroups per learner of its one-launch DQN update (engine_plan.hpp), under the per-call knobs
// FRL_DQN_FUSED=0/1 and FRL_DQN_SPLIT
static LearnFamily learn_family(const frl_engine* e, int batch) { return learn_family(e->h, e->family, batch, env_flag("FRL_DQN_FUSED", true)); }
static int dqn_split_for(const EngineDesc& h, int batch, int pc) { return dqn_split_for(h, batch, pc, env_set("FRL_DQN_SPLIT") ? env_int("FRL_DQN_SPLIT", 0) : -1); }

// frl_learn_path / frl_learn_work / frl_learn_work_executed describe frl_learn(): not the engines that learn through another entry point
// (a PPO engine: frl_learn_path has always said FRL_ERR_INVALID, the work models report no work; a replay-only engine is let through)
static int describes_learn_guard(const EngineDesc& h, const char* who, bool ppo_too) {
    if (h.algo == ALGO_PPO) return ppo_too ? wrong_engine(h, who, FRL_ERR_INVALID) : FRL_OK;
    const char* learn = algo_traits(h.algo).learn;
    return (learn == kFrlLearn || !*learn) ? FRL_OK : wrong_engine(h, who);
}

extern "C" int frl_learn_path(const frl_engine* e, int batch, int* chained_out, int* bytes_out, int* rows_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    const EngineDesc& h = e->h;
    if (const int rc = describes_learn_guard(h, "frl_learn_path", true)) return rc;
    if (batch <= 0 || batch > h.batch_max) return fail(FRL_ERR_INVALID, "batch out of range");
    const LearnPath path = learn_path(h, *e, learn_family(e, batch), batch, dqn_split_for(h, batch, h.P));
    if (chained_out) *chained_out = path.chained;
    if (bytes_out) *bytes_out = path.bytes;
    if (rows_out) *rows_out = path.rows;
    return FRL_OK;
}

extern "C" int frl_actor_park(const frl_engine* e, int* parked_out) {
    if (!e || !parked_out) return fail(FRL_ERR_INVALID, "engine / parked_out is NULL");
    *parked_out = e->family == FAM_CHAINED && e->kern.actor.k == (LearnKernel)ac_actor_v2_kernel;
    return FRL_OK;
}

// -------------------------------------------------------------------------------- launchers
// reduce + clip + Adam (+ soft update) of every unit's net `ad.which`: one fused launch when each net's gradient fits the
// registers of one workgroup, else the two streaming passes
static void launch_adam(frl_engine* e, hipStream_t st, const AdamArgs& ad, int units, dim3 grid_adam) {
    const EngineDesc& h = e->h;
    int max_n4 = 0;
    for (int ag = 0; ag < h.n_agents; ++ag) {
        const int net = (h.algo == ALGO_DQN) ? 0 : (ad.which == 0 ? 2 * ag + 1 : 2 * ag);
        max_n4 = std::max(max_n4, h.net[net].size / 4);
    }
    const bool two_pass = env_set("FRL_ADAM_TWO_PASS");
    if (max_n4 <= kFusedThreads * kFusedVec && !h.noisy && !two_pass) {
        hipLaunchKernelGGL(adam_fused_kernel, dim3(units), dim3(kFusedThreads), 0, st, e->d, ad);
    } else if (max_n4 <= kFusedThreads * kFusedVecWide && !two_pass) {       // (also every NoisyLinear head: the sigma gradients)
        hipLaunchKernelGGL(adam_fused_wide_kernel, dim3(units), dim3(kFusedThreads), 0, st, e->d, ad);
    } else {
        hipLaunchKernelGGL(reduce_kernel, grid_adam, dim3(256), 0, st, e->d, ad);
        hipLaunchKernelGGL(adam_kernel, grid_adam, dim3(256), 0, st, e->d, ad);
    }
}

// One stage of learn() for learners [p0, p0 + pc) on `st`: stage 0 = [draw, obsnorm,] grad(critic | Q) + reduce + adam;
// stage 1 = grad(actor) + reduce + adam; stage 2 = MADDPG's soft update.  The chained families' launches hold their own reduce + Adam.
struct LearnStage {
    hipStream_t st;
    int stage, p0, pc, units;       // units = (learner, agent) pairs
    bool dev_rng, needs_noise;
};

// the head of stage 0 of every family but the one-launch DQN update
static void launch_draw_and_prologue(frl_engine* e, const LearnStage& s, const LearnArgs& a, bool draw) {
    const EngineDesc& h = e->h;
    const dim3 blk(256);
    if (draw) {
        prof_begin(e, PK_DRAW);
        const bool table = a.batch > 256 && 4 * a.batch <= kDrawTableHost && !env_flag("FRL_DRAW_SCAN", false);     // (developer / test knob: no duplicate table)
        const size_t draw_lds = ((size_t)2 * ((a.batch + 3) & ~3) + (table ? 2 * kDrawTableHost : 0)) * sizeof(int);
        hipLaunchKernelGGL(draw_kernel, dim3(s.units), blk, draw_lds, s.st, e->d, a, (s.needs_noise ? 1 : 0) | (table ? 0 : 2));
        prof_end(e);
    }
    if (h.obs_norm_on && h.algo != ALGO_DQN)                         // sample(): norm(obs) updates the statistics first
        hipLaunchKernelGGL(obsnorm_kernel, dim3(s.pc), blk, 0, s.st, e->d, a.batch, 0, s.p0);
    if (h.noisy)      // sets: 0 online on s' (Double only), 1 target on s', 2 online on s
        hipLaunchKernelGGL(noisy_materialise_kernel, dim3(h.P), blk, 0, s.st, e->d, 0, 3, 0x2);
}

// kernels_dqn2.hip: draw + update + Adam + soft update in one launch (`step`, frl_rollout: add() and the next select_action too)
static void launch_dqn_fused(frl_engine* e, const LearnStage& s, LearnArgs a, const DqnStepArgs* step) {
    a.dqn_split = dqn_split_for(e->h, a.batch, s.pc);
    prof_begin(e, PK_GRAD_CRITIC);
    const DqnStepArgs sa = step ? *step : DqnStepArgs{};
    hipLaunchKernelGGL(e->kern.critic.kd, dim3(s.pc * a.dqn_split), dim3(256), (size_t)e->kern.lds_bytes, s.st, e->d, a, sa);
    prof_end(e);
}

// One update on the row-chunk launch shape (rowchunk_layout.h): the gradient kernel over units x ns workgroups on the 8-aligned grid
// (a unit's slices on one XCD), then reduce + clip + Adam of the units' net ad.which (1: the actor slots, 0: the critic's).  The caller
// brings the kernel's own arguments and ad's hyper-parameters; the launch shape's fields of ad are set here.
template <class Kernel, class... Args>
static void launch_rowchunk_update(frl_engine* e, hipStream_t st, int units, int p0, int ns, AdamArgs ad, Kernel k, const Args&... args) {
    const bool actor = ad.which == 1;
    prof_begin(e, actor ? PK_GRAD_ACTOR : PK_GRAD_CRITIC);
    hipLaunchKernelGGL(k, dim3(((units + 7) / 8) * 8 * ns), dim3(256), e->lds_bytes, st, e->d, args..., ns);
    prof_end(e);
    ad.ns = ns; ad.p0 = p0; ad.G = e->h.Gmax;
    prof_begin(e, actor ? PK_ADAM_ACTOR : PK_ADAM_CRITIC);
    launch_adam(e, st, ad, units, dim3(units * e->h.Gmax));      // (a NoisyLinear head's sigma gradients are derived in its slab sums)
    prof_end(e);
}
// what frl_learn's row-chunk families hand their Adam launches out of the call's arguments
static AdamArgs learn_adam_args(const LearnArgs& a, bool actor) {
    AdamArgs ad{};
    ad.which = actor ? 1 : 0; ad.lr = actor ? a.actor_lr : a.critic_lr;
    ad.batch = a.batch; ad.eps = a.adam_eps; ad.beta1 = a.beta1; ad.beta2 = a.beta2; ad.clip = a.clip_norm; ad.tau = a.tau; ad.alpha_lr = a.alpha_lr;
    return ad;
}

// the row-chunk kernels of DQN / C51 / DDPG / TD3 / SAC / MADDPG / discrete SAC, and FAM_ATT's own (e->kern) on the same launch shape
// (what launch_att forwarded to: FAM_ATT's case of launch_learn_stage calls this directly)
static void launch_rowchunk(frl_engine* e, const LearnStage& s, const LearnArgs& a, LearnFamily fam) {
    const EngineDesc& h = e->h;
    const bool actor = s.stage == 1, sac = h.algo == ALGO_SAC || h.algo == ALGO_SAC_DISCRETE, maddpg = is_maddpg(h.algo);
    auto k = actor ? (h.algo == ALGO_SAC_DISCRETE ? sacd_actor_kernel : ac_actor_kernel)
                   : (h.algo == ALGO_DQN ? (h.c51_atoms ? c51_grad_kernel : dqn_grad_kernel) : h.algo == ALGO_SAC_DISCRETE ? sacd_critic_kernel : ac_critic_kernel);
    if (fam == FAM_ATT) k = actor ? e->kern.actor.kr : e->kern.critic.kr;
    AdamArgs ad = learn_adam_args(a, actor);
    ad.target_entropy = a.target_entropy;
    if (actor) {
        ad.soft = maddpg ? 0 : 1; ad.sac_alpha = sac ? 1 : 0;
    } else {
        ad.wd = a.critic_wd;
        ad.soft = (h.algo == ALGO_DQN) ? 1 : ((!maddpg && a.do_actor) ? 1 : 0);
    }
    launch_rowchunk_update(e, s.st, s.units, s.p0, rowchunk_ns(h, a.batch), ad, k, a);
}

// kernels_critic2.hip / kernels_actor2.hip: a whole stage of DDPG / TD3 / SAC in one launch, one workgroup per learner
static void launch_chained(frl_engine* e, const LearnStage& s, LearnArgs a) {
    const LearnKernels& K = e->kern;
    LearnKernel k = K.actor.k;
    if (s.stage == 0) {
        a.stagger = env_int("FRL_STAGGER", 0);         // developer knob: spread the Adam bursts of the first round
        a.stagger_groups = env_int("FRL_STAGGER_GROUPS", 4); a.stagger_wgs = e->n_cus;
        // (_nv: next_obs 16-byte aligned with its 16 columns inside the row, (reward, done) an aligned pair)
        const RecordDesc& R = e->h.rec;
        const bool nv = R.nobs_off[0] % 4 == 0 && R.nobs_off[0] + 16 <= R.stride && R.rew_off % 2 == 0 && R.done_off == R.rew_off + 1 && !env_set("FRL_CRITIC2_NOVEC");
        k = (nv && K.critic_nv.k) ? K.critic_nv.k : K.critic.k;
    }
    prof_begin(e, s.stage == 0 ? PK_GRAD_CRITIC : PK_GRAD_ACTOR);
    hipLaunchKernelGGL(k, dim3(s.pc), dim3(K.block), (size_t)K.lds_bytes, s.st, e->d, a);
    prof_end(e);
}

// kernels_criticw.hip / kernels_actorw.hip (hidden 256: kernels_criticx.hip / kernels_actorx.hip): one workgroup per (learner, agent)
static void launch_wide(frl_engine* e, const LearnStage& s, const LearnArgs& a) {
    const LearnKernels& K = e->kern;
    prof_begin(e, s.stage == 0 ? PK_GRAD_CRITIC : PK_GRAD_ACTOR);
    hipLaunchKernelGGL(s.stage == 0 ? K.critic.k : K.actor.k, dim3(s.units), dim3(K.block), (size_t)K.lds_bytes, s.st, e->d, a);
    prof_end(e);
}

// what every kernels_solo.hip / kernels_solow.hip launch takes; the launch is one more epoch of the learners' counting barriers
static SoloArgs solo_args(frl_engine* e) {
    SoloArgs sa{e->d_solo_slab, e->d_solo_part, e->d_solo_bar, e->d_solo_err, e->solo_bar_base, e->solo_stride, nullptr, nullptr, 0ull};
    if (e->h.solow) { sa.tiles = e->h.solow; sa.bar2 = e->d_solow_bar2; sa.row_wgs = e->solow_row_wgs; sa.update_wgs = e->solow_wgs; }
    e->solo_bar_base += kSoloWG;
    return sa;
}

// The next call's rows drawn by spare workgroups of this critic launch: two alternating slots of `slot_stride` ints, a tag the reader
// checks (stale or foreign tags fail the kernel's check, and it draws for itself).  The launch reads slot seq & 1 and, where it may,
// writes the other one for the counter the next frl_learn takes, unless something else draws first.  -> whether it writes
static bool predraw_slots(frl_engine* e, SoloArgs& sa, size_t slot_stride, bool read, bool may_write) {
    if (read) sa.pre_read = e->d_solo_pre + (size_t)(e->solo_pre_seq & 1) * slot_stride;
    if (may_write) {
        sa.pre_write = e->d_solo_pre + (size_t)((e->solo_pre_seq + 1) & 1) * slot_stride;
        sa.pre_counter = e->rng_counter;
    }
    ++e->solo_pre_seq;
    return may_write;
}

// kernels_solo.hip: sixteen (eight) workgroups per learner, reduce + Adam behind grid barriers (`sstep`, frl_rollout: the vector step folded in)
static void launch_solo(frl_engine* e, const LearnStage& s, const LearnArgs& a, const SoloStepArgs* sstep) {
    const LearnKernels& K = e->kern;
    const int P = e->h.P, W = e->h.solo;
    prof_begin(e, s.stage == 0 ? PK_GRAD_CRITIC : PK_GRAD_ACTOR);
    SoloArgs sa = solo_args(e);
    const SoloStepArgs ss = sstep ? *sstep : SoloStepArgs{};
    int extra = 0;
    if (s.stage == 0) {
        // the next call's rows drawn by pc spare workgroups of this launch (plain frl_learn calls with device draws; the spare ones
        // need a CU of their own — 117 KB of LDS — next to the learners' pc x 16: FRL_SOLO_PREDRAW=0/1 overrides)
        const bool predraw_on = env_flag("FRL_SOLO_PREDRAW", true);
        if (s.dev_rng && !sstep && e->d_solo_pre && s.pc == P && predraw_slots(e, sa, (size_t)P * kSoloPre, true, s.pc * (W + 1) <= e->n_cus && predraw_on))
            extra = s.pc;
    }
    hipLaunchKernelGGL(s.stage == 0 ? K.critic.ks : K.actor.ks, dim3(s.pc * W + extra), dim3(K.block), (size_t)K.lds_bytes, s.st, e->d, a, sa, ss);
    prof_end(e);
}

// kernels_solow.hip: sixteen workgroups (+ helpers) per unit, W1 streamed from the block.  ma_predraw: a multi-agent call whose rows
// spare workgroups may draw a launch ahead; ma_use_pre: ... and the previous launch did, for exactly this call (the dispatcher skipped draw_kernel)
static void launch_solow(frl_engine* e, const LearnStage& s, const LearnArgs& a, bool ma_predraw, bool ma_use_pre) {
    const EngineDesc& h = e->h;
    const LearnKernels& K = e->kern;
    prof_begin(e, s.stage == 0 ? PK_GRAD_CRITIC : PK_GRAD_ACTOR);
    SoloArgs sa = solo_args(e);
    SolowKernel k = K.actor.kw;
    int extra = 0;
    if (s.stage == 0) {
        const bool predraw_on = env_flag("FRL_SOLO_PREDRAW", true);
        if (h.n_agents == 1) {      // the learners' first helper workgroups draw
            if (s.dev_rng && e->d_solo_pre && s.pc == h.P) predraw_slots(e, sa, (size_t)h.P * kSoloPre, true, e->solow_wgs > e->solow_row_wgs && predraw_on);
        } else {                    // one spare workgroup per unit draws, the duplicate table in its own LDS
            e->ma_pre_valid = predraw_slots(e, sa, (size_t)h.P * h.n_agents * (8 + h.batch_max), ma_use_pre,
                                            ma_predraw && s.units * (e->solow_wgs + 1) <= e->n_cus && predraw_on);
            if (e->ma_pre_valid) { extra = s.units; e->ma_pre_counter = sa.pre_counter; e->ma_pre_size = a.size; e->ma_pre_batch = a.batch; }
        }
        k = a.fuse_actor ? K.step.kw : K.critic.kw;
    }
    hipLaunchKernelGGL(k, dim3(s.units * e->solow_wgs + extra), dim3(K.block), (size_t)K.lds_bytes, s.st, e->d, a, sa);
    prof_end(e);
}

// kernels_masac.hip.  Stage 0: every (learner, agent) critic unit in one launch, then their reduce + clip + Adam (targets untouched: the soft
// stage moves them).  Stage 1, once per agent in agent order (a.agent): the actor launch over LEARNERS for that agent, its reduce + clip +
// Adam and the agent's alpha step — stream order makes agent i's launch read the actors of agents j < i as stepped (MASAC.py:221,254)
static void launch_masac(frl_engine* e, const LearnStage& s, const LearnArgs& a) {
    const bool actor = s.stage == 1;
    AdamArgs ad = learn_adam_args(a, actor);
    if (actor) { ad.sac_alpha = 2; ad.agent1 = a.agent + 1; }
    launch_rowchunk_update(e, s.st, actor ? s.pc : s.units, s.p0, rowchunk_ns(e->h, a.batch), ad, actor ? e->kern.actor.kr : e->kern.critic.kr, a);
}

static void launch_learn_stage(frl_engine* e, hipStream_t st, LearnFamily fam, LearnArgs a, int stage, int p0, int pc, bool dev_rng, bool needs_noise,
                               const DqnStepArgs* step = nullptr, const SoloStepArgs* sstep = nullptr) {
    const EngineDesc& h = e->h;
    a.p0 = p0; a.p_count = pc;
    const LearnStage s{st, stage, p0, pc, pc * h.n_agents, dev_rng, needs_noise};
    if (stage == 2) {                                 // MATD3_simple.py:245-246: targets move with the delayed policy step
        prof_begin(e, PK_SOFT);
        int biggest = 0;
        for (int i = 0; i < h.n_nets; ++i) biggest = std::max(biggest, h.net[i].size);
        const int per = std::max(1, std::min((biggest + 4095) / 4096, 4 * e->n_cus / std::max(1, pc * h.n_nets)));
        hipLaunchKernelGGL(soft_update_kernel, dim3(pc * h.n_nets, per), dim3(256), 0, st, e->d, a.tau, p0);
        prof_end(e);
        return;
    }
    if (fam == FAM_DQN_FUSED) { launch_dqn_fused(e, s, a, step); return; }
    // kernels_solow.hip, MADDPG without smoothing noise: the rows may have been drawn by the previous launch's spare workgroups (one per
    // unit) — for exactly this counter, ring size and batch, or draw_kernel runs as ever
    const bool ma_predraw = fam == FAM_SOLOW && h.n_agents > 1 && stage == 0 && dev_rng && !needs_noise && pc == h.P;
    const bool ma_use_pre = ma_predraw && e->ma_pre_valid && e->ma_pre_counter == a.rng_counter && e->ma_pre_size == a.size && e->ma_pre_batch == a.batch;
    if (stage == 0) {
        const bool draws_in_critic = fam == FAM_SOLO || (fam == FAM_SOLOW && h.n_agents == 1);      // (kernels_solo.hip / single-agent kernels_solow.hip)
        launch_draw_and_prologue(e, s, a, dev_rng && !ma_use_pre && !draws_in_critic);
    }
    switch (fam) {
        case FAM_ROWCHUNK: case FAM_ATT: launch_rowchunk(e, s, a, fam); break;
        case FAM_CHAINED: launch_chained(e, s, a); break;
        case FAM_SOLO: launch_solo(e, s, a, sstep); break;
        case FAM_SOLOW: launch_solow(e, s, a, ma_predraw, ma_use_pre); break;
        case FAM_WIDE: case FAM_WIDE16: launch_wide(e, s, a); break;
        case FAM_MASAC: launch_masac(e, s, a); break;
        case FAM_DQN_FUSED: break;
    }
}

// What frl_rollout folds into a learn step (nullptr: a plain frl_learn).  dqn (DQN engines on the fused path) / solo (kernels_solo.hip): the
// vector step's add() and the next select_action in the same launches.  size_at_launch >= 0: the rings' common size WHEN THE LAUNCH RUNS (a
// pre-armed launch is enqueued before the step's rows are counted in e->size).  stream: non-null for the pool's second stream
struct StepFold { const DqnStepArgs* dqn; const SoloStepArgs* solo; int size_at_launch; hipStream_t stream; };
static int learn_impl(frl_engine* e, const frl_learn_args* args, const StepFold* fold) {
    const DqnStepArgs* step = fold ? fold->dqn : nullptr;
    const SoloStepArgs* sstep = fold ? fold->solo : nullptr;
    const int size_override = fold ? fold->size_at_launch : -1;
    hipStream_t stream_override = fold ? fold->stream : nullptr;
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (algo_traits(h.algo).learn != kFrlLearn) return wrong_engine(h, "frl_learn");
    if (args->batch < 1 || args->batch > h.batch_max) return fail(FRL_ERR_INVALID, "batch %d outside [1,%d]", args->batch, h.batch_max);
    int min_size = h.capacity;
    for (int p = 0; p < h.P; ++p) min_size = std::min(min_size, e->size[p]);
    if (size_override >= 0) min_size = size_override;
    if (min_size < args->batch) return fail(FRL_ERR_STATE, "a ring holds %d rows < batch %d", min_size, args->batch);
    if (args->per && (h.algo != ALGO_DQN || !e->per_on)) return fail(FRL_ERR_STATE, "per = 1 needs a DQN engine with frl_per_enable");
    if (args->per && args->idx) return fail(FRL_ERR_INVALID, "per = 1 uses the rows of the last frl_per_sample; idx must be NULL");
    const bool dev_rng = (args->idx == nullptr) && !args->per;
    if (dev_rng && min_size < 2 * args->batch)
        return fail(FRL_ERR_STATE, "device index draw needs len(buffer) >= 2*batch (have %d); pass idx", min_size);
    const bool td3_like = (h.algo == ALGO_TD3 || is_maddpg(h.algo));           // MADDPG + noise/delay = MATD3_simple.py (ATT-MADDPG: do_actor only)
    const bool needs_noise = (h.algo == ALGO_SAC) || h.algo == ALGO_MASAC || (td3_like && args->use_policy_noise);
    if (h.algo == ALGO_MASAC && args->use_policy_noise) return fail(FRL_ERR_STATE, "frl_learn: MASAC has no target policy smoothing (MATD3's): use_policy_noise must be 0");
    if (h.algo == ALGO_MASAC && args->loss_kind == FRL_LOSS_HUBER) return fail(FRL_ERR_INVALID, "MASAC's critic loss is F.mse_loss (MASAC.py:241): no Huber variant");
    if (h.algo == ALGO_MADDPG_ATT && args->use_policy_noise) return fail(FRL_ERR_INVALID, "ATT-MADDPG has no target policy smoothing: use_policy_noise must be 0");
    if (!dev_rng && needs_noise && !args->noise) return fail(FRL_ERR_INVALID, "idx given without noise: both or neither");
    int rc = flush_stage(e);
    if (rc) return rc;
    rc = upload_idx_noise(e, args->idx, needs_noise ? args->noise : nullptr, args->batch, h.n_agents);
    if (rc) return rc;
    LearnArgs a;
    memset(&a, 0, sizeof a);
    a.batch = args->batch;
    a.size = min_size;
    a.device_rng = dev_rng ? 1 : 0;
    a.do_actor = td3_like ? (args->do_actor ? 1 : 0) : 1;
    a.gamma = args->gamma; a.tau = args->tau;
    a.actor_lr = args->actor_lr; a.critic_lr = args->critic_lr; a.alpha_lr = args->alpha_lr;
    a.adam_eps = args->adam_eps > 0 ? args->adam_eps : 1e-8f;
    a.beta1 = 0.9f; a.beta2 = 0.999f;
    a.critic_wd = args->critic_weight_decay;
    a.clip_norm = args->clip_norm;
    a.policy_noise = args->policy_noise; a.noise_clip = args->noise_clip;
    a.max_action = args->max_action != 0.f ? args->max_action : 1.f;
    a.policy_noise_scale = args->policy_noise_scale;
    a.use_policy_noise = (td3_like && args->use_policy_noise) ? 1 : 0;
    a.target_entropy = args->target_entropy;
    a.double_dqn = (h.algo == ALGO_DQN && args->double_dqn) ? 1 : 0;
    a.use_isw = (h.algo == ALGO_DQN && args->per) ? (args->per == 2 ? 2 : 1) : 0;
    if (args->loss_kind != FRL_LOSS_MSE && args->loss_kind != FRL_LOSS_HUBER) return fail(FRL_ERR_INVALID, "unknown loss_kind %d", args->loss_kind);
    if (args->loss_kind == FRL_LOSS_HUBER) {
        if (!(args->huber_delta > 0.f)) return fail(FRL_ERR_INVALID, "Huber loss needs huber_delta > 0");
        if (h.c51_atoms) return fail(FRL_ERR_STATE, "the Categorical head's loss is a cross-entropy: no Huber variant");
        if (h.algo == ALGO_SAC_DISCRETE) return fail(FRL_ERR_INVALID, "discrete SAC's critic loss is F.mse_loss (SAC_add_discrete.py:313-314): no Huber variant");
        a.huber = 1; a.huber_delta = args->huber_delta;
    }
    a.rng_counter = e->rng_counter++;
    ++e->param_version;                       // (select_action's re-laid-out copies of the nets are stale from here on)
    // One chain for the whole population.  Measured and rejected (profiles/README.md): two halves of the population on two
    // streams so that one half's HBM-bound reduce/Adam runs under the other half's MFMA-bound gradient kernel — unchained
    // +2.7 %, with the gradient kernels chained across the streams -8 %: the Adam workgroups do not get co-resident with
    // the gradient kernel's (2 x 80 KB of LDS and 448 of 512 VGPRs per SIMD are taken).
    const LearnFamily fam = learn_family(e, a.batch);
    // (kernels_solow.hip moves MADDPG's targets at the end of its actor launch)
    const bool actor_stage = (h.algo != ALGO_DQN && a.do_actor), soft_stage = (is_maddpg(h.algo) && a.do_actor && fam != FAM_SOLOW);
    if (h.noisy) {
        // the reference draws noise per forward in program order: [online(s') if Double,] target(s'), online(s)
        const int first = a.double_dqn ? 0 : 1;
        if (args->noisy_eps) { rc = noisy_upload(e, args->noisy_eps, first, 3 - first); if (rc) return rc; }
        else hipLaunchKernelGGL(noisy_draw_kernel, dim3(h.P, 3), dim3(256), 0, e->stream, e->d, 0, 3, e->rng_counter++);
    }
    // kernels_solow.hip, single agent, helper workgroups present: a policy step is ONE launch — the critic's update runs on the helpers
    // under the policy's forward (FRL_SOLOW_FUSE=0: two launches)
    if (actor_stage && fam == FAM_SOLOW && h.n_agents == 1 && e->solow_wgs > e->solow_row_wgs) a.fuse_actor = env_flag("FRL_SOLOW_FUSE", true) ? 1 : 0;
    hipStream_t lst = stream_override ? stream_override : e->stream;      // (frl_rollout's pre-armed launches: the pool's second stream)
    // frl_rollout on a solo engine (`sstep`): the step's add() rides at the head of the critic launch, its tail (obs advance + the next
    // select_action + hand-over) at the end of the step's LAST launch
    SoloStepArgs s0, s1;
    if (sstep) {
        if (fam != FAM_SOLO || !dev_rng) return fail(FRL_ERR_STATE, "step fusion needs a solo engine with device draws");
        s0 = s1 = *sstep;
        s0.head = 1; s0.tail = actor_stage ? 0 : 1;
        s1.head = 0; s1.tail = 1;
    }
    launch_learn_stage(e, lst, fam, a, 0, 0, h.P, dev_rng, needs_noise, step, sstep ? &s0 : nullptr);
    if (fam == FAM_MASAC) {      // DESIGN.md "MASAC": behind all the critics the agents' actor + alpha steps one after the other, then every target
        for (int ag = 0; ag < h.n_agents; ++ag) { a.agent = ag; launch_learn_stage(e, lst, fam, a, 1, 0, h.P, dev_rng, needs_noise); }
    } else if (actor_stage && !a.fuse_actor) {
        launch_learn_stage(e, lst, fam, a, 1, 0, h.P, dev_rng, needs_noise, nullptr, sstep ? &s1 : nullptr);
    }
    if (soft_stage || fam == FAM_MASAC) launch_learn_stage(e, lst, fam, a, 2, 0, h.P, dev_rng, needs_noise);
    HIP_TRY(hipGetLastError());
    if (sstep) return FRL_OK;
    if (args->stats_out) return frl_stats_get(e, args->stats_out);
    return FRL_OK;
}

extern "C" int frl_learn(frl_engine* e, const frl_learn_args* args) { return learn_impl(e, args, nullptr); }

// ------------------------------------------------------------------------------ work models
// Algorithmic work of one launch (DESIGN.md "Roofline"): flops = 2*B*sum(in*out) per forward
// pass, x2 more per backward pass that needs both dX and dW, x1 for dX-only passes; bytes =
// gathered records + 24 B per trained parameter (theta, m, v read+write) + 8 B per
// soft-updated target parameter (SURVEY.md §8d).
// `executed` (include/freerl_hip.h): the flops the launch executes — no first-layer dX for trained nets, the agent's action columns
// only for dQ/da.  Per (learner, agent): target actors fwd + target critic fwd + critic fwd + dW (all layers) + dX (layers 2..);
// actor stage: actor fwd + dW + dX (layers 2..) + per Q head used by the policy loss fwd + dX (layers 2.. whole, layer 1 x act_dim).
// (every flop term is an integer well below 2^53: the sums are exact in whatever order they are taken)
static void learn_work_model(const EngineDesc& h, int batch, int do_actor, bool executed, double* flops_out, double* bytes_out) {
    auto macs = [](const NetDesc& N, int l0, int nl) { double s = 0; for (int i = l0; i < l0 + nl; ++i) s += (double)N.L[i].n * N.L[i].k; return s; };
    auto all = [&](const NetDesc& N) { return macs(N, 0, N.n_layers); };
    auto first = [](const NetDesc& N) {            // the first layers of all heads
        const int nl = N.n_layers / std::max(1, N.heads);
        double s = 0;
        for (int hd = 0; hd < N.heads; ++hd) s += (double)N.L[hd * nl].n * N.L[hd * nl].k;
        return s;
    };
    auto train = [&](const NetDesc& N) { return 3 * all(N) - (executed ? first(N) : 0.0); };      // fwd + dW + dX
    double fl = 0, by = 0;
    const double B = batch;
    const RecordDesc& R = h.rec;
    if (h.algo == ALGO_DQN) {
        const NetDesc& N = h.net[0];
        fl = 2 * B * (all(N) + train(N));              // target fwd, online fwd + bwd
        by = 4 * B * (2 * R.obs_total + R.act_total + 2) + 24.0 * N.n_params + 8.0 * N.n_params;
    } else if (h.algo == ALGO_SAC_DISCRETE) {
        // kernels_sacd.hip: online actor fwd on s', target critic fwd (both heads) on s', critic fwd + bwd;
        // actor stage: critic fwd (both heads, no backward), actor fwd + bwd.  No target-actor pass, no dX through the critic
        const NetDesc &NA = h.net[0], &NC = h.net[1];
        double f = all(NA) + all(NC) + train(NC);
        by = 4 * B * (2 * R.obs_total + R.act_total + 2) + 24.0 * NC.n_params;
        if (do_actor) {
            f += all(NC) + train(NA);
            by += 4 * B * R.obs_total + 24.0 * NA.n_params + 8.0 * (NA.n_params + NC.n_params);
        }
        fl = 2 * B * f;
    } else if (h.algo != ALGO_PPO) {
        const int n = h.n_agents;
        for (int ag = 0; ag < n; ++ag) {
            const NetDesc &NC = h.net[2 * ag + 1], &NA = h.net[2 * ag];
            const int ql = NC.n_layers / NC.heads;
            double f = 0;
            for (int j = 0; j < n; ++j) f += all(h.net[2 * j]);      // target actors fwd
            f += all(NC) + train(NC);                               // target critic heads fwd, critic fwd + bwd
            double bytes = 4 * B * n * (2.0 * R.obs_total / n + R.act_total / (double)n + 2) + 24.0 * NC.n_params;
            if (do_actor) {
                const int nq = (h.algo == ALGO_SAC) ? NC.heads : 1;
                f += train(NA);                                     // actor fwd + bwd
                // Q(s, pi(s)) fwd + dX-only bwd
                f += nq * (macs(NC, 0, ql) + (executed ? macs(NC, 1, ql - 1) + (double)NC.L[0].n * R.act_dim[ag] : macs(NC, 0, ql)));
                bytes += 24.0 * NA.n_params + 8.0 * (NA.n_params + NC.n_params);
            }
            fl += 2 * B * f;
            by += bytes;
        }
    }
    if (flops_out) *flops_out = fl * h.P;
    if (bytes_out) *bytes_out = by * h.P;
}

extern "C" int frl_learn_work(const frl_engine* e, int batch, int do_actor, double* flops_out, double* bytes_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    if (const int rc = describes_learn_guard(e->h, "frl_learn_work", false)) return rc;
    learn_work_model(e->h, batch, do_actor, false, flops_out, bytes_out);
    return FRL_OK;
}

extern "C" int frl_learn_work_executed(const frl_engine* e, int batch, int do_actor, double* flops_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    if (const int rc = describes_learn_guard(e->h, "frl_learn_work_executed", false)) return rc;
    learn_work_model(e->h, batch, do_actor, true, flops_out, nullptr);
    return FRL_OK;
}
