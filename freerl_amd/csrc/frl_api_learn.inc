// frl_learn(): which kernel family an engine learns with, the ONE table of the families' kernels and LDS bytes (a new family is
// registered there), a launcher per family, learn_impl and the work models.  Part of frl_api.hip.

// ------------------------------------------------------------------------- shape predicates
// One learner per workgroup, register-chained, Adam fused (kernels_critic2.hip / kernels_actor2.hip): the reference's standard
// narrow shape at populations that give every CU a learner; everything else takes the row-chunk kernels + reduce / Adam
// launches.  The family is chosen ONCE, at frl_create (chained_shape + population, FRL_CRITIC_V2=0/1 overrides the population
// threshold — the tests run both families on the same inputs): the chained kernels keep the nets in fragment-image order in
// HBM (NetDesc::frag), which the row-chunk kernels do not read.
static bool chained_shape(const EngineDesc& h) {
    const NetDesc &NA0 = h.net[0], &NC0 = h.net[1];
    auto packed = [](const NetDesc& N) {          // every head block at the offsets the kernels hard-code (frl_desc.h: kL1w ...)
        for (int hd = 0; hd < N.heads; ++hd) {
            const LayerDesc* L = N.L + 3 * hd;
            const int b = hd * kHeadFloats;
            if (L[0].w_off != b + kL1w || L[0].b_off != b + kL1b || L[1].w_off != b + kL2w || L[1].b_off != b + kL2b ||
                L[2].w_off != b + kL3w || L[2].b_off != b + kL3b) return false;
        }
        return N.extra_n == 0 || (N.heads == 1 && N.extra_off == kHeadFloats);
    };
    if (NA0.n_layers != 3 || NC0.n_layers != 3 * NC0.heads || h.hidden != 128 || !packed(NA0) || !packed(NC0)) return false;
    // ([s | a] as one aligned slice of the record: the chained kernels read a lane's four columns of it as one dwordx4)
    if (h.rec.obs_off[0] % 4 != 0 || h.rec.act_off[0] != h.rec.obs_off[0] + h.rec.obs_dim[0] || h.rec.obs_off[0] + 16 > h.rec.stride) return false;
    return (h.algo == ALGO_DDPG || h.algo == ALGO_TD3 || h.algo == ALGO_SAC) && h.n_agents == 1 &&
           NA0.L[0].k_pad == 16 && NC0.L[0].k_pad == 16 && h.rec.act_dim[0] <= 4 && NA0.L[2].n_pad == 16 &&
           h.batch_max <= 256 && NA0.hidden_act == ACT_RELU && NC0.hidden_act == ACT_RELU;
}
// The K-sliced chained family (device/chain_wide.hpp): the reference's hidden-128 ReLU actor-critic nets with first layers of up
// to 416 input columns and actor heads of up to 32 outputs that chained_shape() does not admit — SAC / TD3 / DDPG on wide
// observations (config 4: Humanoid's 376 + 17), MADDPG_simple's per-agent actors and centralised critics (config 5).
// MATD3 (MATD3_simple.py:195-262) is the same launch pair with twin critics, set j of the unit's noise on agent j's target action
// and the host's delayed actor / soft-update stages.
static bool wide_shape(const EngineDesc& h) {
    const bool single = (h.algo == ALGO_DDPG || h.algo == ALGO_TD3 || h.algo == ALGO_SAC) && h.n_agents == 1;
    const bool multi = h.algo == ALGO_MADDPG && h.n_agents >= 1;
    const int H = h.hidden;                    // 128: chain_wide.hpp; 256: chain_wide16.hpp
    if (!(single || multi) || (H != 128 && H != 256) || h.rec.act_total > kWideApitch) return false;
    // WideNet::stage_idx (chain_wide.hpp; also the hidden-256 kernels') copies the batch's ring indices into the 64 KB LDS union:
    // 2 * kWideSlice = 16384 ints.  Larger batches stay with the row-chunk family.
    if (h.batch_max > 2 * kWideSlice) return false;
    const int nt3 = h.net[0].L[2].n_pad;
    for (int j = 0; j < h.n_agents; ++j) {
        const NetDesc &NA0 = h.net[2 * j], &NC0 = h.net[2 * j + 1];
        if (NA0.n_layers != 3 || NA0.heads != 1 || NC0.n_layers != 3 * NC0.heads || NC0.heads != h.net[1].heads) return false;
        if (NA0.hidden_act != ACT_RELU || NC0.hidden_act != ACT_RELU) return false;
        if (NA0.L[0].k_pad > 16 * kWideMaxKB1 || NC0.L[0].k_pad > 16 * kWideMaxKB1) return false;
        if (NA0.L[2].n_pad != nt3 || nt3 > 32) return false;                 // one head-tile count for every agent's actor
        for (int hd = 0; hd < NC0.heads; ++hd)
            if (NC0.L[3 * hd].n_pad != H || NC0.L[3 * hd + 1].n_pad != H || NC0.L[3 * hd + 1].k_pad != H || NC0.L[3 * hd + 2].n_pad != 16) return false;
        if (NA0.L[0].n_pad != H || NA0.L[1].n_pad != H || NA0.L[1].k_pad != H) return false;
    }
    return true;
}
// kernels_dqn2.hip: the reference's Q-net (obs -> 128 -> n_actions, or the Dueling [V ; A] head) with the TD update of DQN.py and
// DQN_with_tricks.py's Double / PER-weighted variants (PER's importance weights, mean or per-row, are applied in the launch); Noisy and
// Categorical heads take the row-chunk chain.
static bool dqn_fused_shape(const EngineDesc& h, int batch) {
    const NetDesc& N = h.net[0];
    return h.algo == ALGO_DQN && !h.noisy && !h.c51_atoms && h.hidden == 128 && N.n_layers == 2 &&
           N.L[0].k_pad == 16 && N.L[1].n_pad == 16 && batch <= kDqn2Batch && !h.obs_norm_on && N.hidden_act == ACT_RELU;
}

// --------------------------------------------------------------------------- the family table
enum LearnKernelStage { LK_CRITIC, LK_CRITIC_NV, LK_ACTOR, LK_STEP };
struct LearnKernelRow {
    LearnFamily fam;
    int stage;          // LK_CRITIC_NV: the 8-wave chained critic with aligned next_obs / (reward, done) loads; LK_STEP: a whole policy step
    int sub;            // FAM_CHAINED: waves per workgroup; FAM_SOLO: workgroups per learner; FAM_SOLOW: 1 single-agent, 2 (learner, agent) units
    int lds_bytes;      // dynamic LDS of the launch = the kernels' hipFuncAttributeMaxDynamicSharedMemorySize
    KernelPtr k[2][2];  // [critic heads - 1][16-column tiles of the actor head - 1]
};
constexpr int kLdsChain4 = critic2_lds_floats() * (int)sizeof(float), kLdsChain8 = critic8_lds_floats() * (int)sizeof(float);
constexpr int kLdsSolo = std::max(solo_lds_floats(), critic2_lds_floats()) * (int)sizeof(float);      // (critic2: the rollout tail's act_frag_body)
constexpr int kLdsSolow = solow_lds_floats() * (int)sizeof(float);
constexpr int kLdsWide = wide_lds_floats() * (int)sizeof(float), kLdsWide16 = wide16_lds_floats_host() * (int)sizeof(float);
static const LearnKernelRow kLearnKernels[] = {
    {FAM_DQN_FUSED, LK_CRITIC, 0, dqn2_lds_floats() * (int)sizeof(float), {{dqn_fused_kernel, dqn_fused_kernel}, {dqn_fused_kernel, dqn_fused_kernel}}},
    // the register-chained family: one workgroup per learner with the nets as LDS images (156 KB)
    {FAM_CHAINED, LK_CRITIC, 8, kLdsChain8, {{ac_critic_v2_single_kernel, ac_critic_v2_single_kernel}, {ac_critic_v2_twin_kernel, ac_critic_v2_twin_kernel}}},
    {FAM_CHAINED, LK_CRITIC_NV, 8, kLdsChain8, {{ac_critic_v2_single_nv_kernel, ac_critic_v2_single_nv_kernel}, {ac_critic_v2_twin_nv_kernel, ac_critic_v2_twin_nv_kernel}}},
    {FAM_CHAINED, LK_ACTOR, 8, kLdsChain8, {{ac_actor_v2_kernel, ac_actor_v2_kernel}, {ac_actor_v2_kernel, ac_actor_v2_kernel}}},
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
static LearnKernels resolve_learn_kernels(LearnFamily fam, int chain_waves, const EngineDesc& h) {
    const int twin = h.net[1].heads == 2, a2 = h.net[0].L[2].n_pad > 16;
    const int sub = fam == FAM_CHAINED ? chain_waves : fam == FAM_SOLO ? h.solo : fam == FAM_SOLOW ? (h.n_agents > 1 ? 2 : 1) : 0;
    LearnKernels K;
    K.block = (fam == FAM_CHAINED && sub == 8) ? 512 : 256;
    for (const LearnKernelRow& r : kLearnKernels) {
        if (r.fam != fam || r.sub != sub) continue;
        (r.stage == LK_CRITIC ? K.critic : r.stage == LK_CRITIC_NV ? K.critic_nv : r.stage == LK_ACTOR ? K.actor : K.step) = r.k[twin][a2];
        K.lds_bytes = r.lds_bytes;
    }
    return K;
}

// ------------------------------------------------------------------------- family selection
// The chained family of the engine (and with it the parameter layout in HBM), fixed for the engine's life: sets h.solo / h.solow /
// h.wide (+ its scratch geometry), NetDesc::frag and e->solow_row_wgs.  FAM_ROWCHUNK: none.
static LearnFamily choose_engine_family(frl_engine* e) {
    EngineDesc& h = e->h;
    if (!e->has_nets) return FAM_ROWCHUNK;
    // (FRL_SOLOW_NARROW=1, developer knob: the narrow standard shape on kernels_solow.hip — one first-layer k-tile — for A/Bs against kernels_solo.hip)
    if (chained_shape(h) && !env_flag("FRL_SOLOW_NARROW", false)) {
        const bool named = env_set("FRL_CRITIC_V2");
        // measured (bench workload, updates/s): 128 learners are exactly one round of the row-chunk kernels' 512 resident
        // workgroups — 484 k against 373 k for 128 one-learner workgroups on half the CUs; from 129 up the chained kernels win
        // (160: 459 k / 393 k, 256: 694 k / 566 k) or tie (320: 472 k / 480 k)
        // up to kSoloMaxP learners: one learner on sixteen workgroups (kernels_solo.hip; FRL_SOLO=0/1 overrides, FRL_CRITIC_V2 set
        // means the caller asked for one of the other two families by name)
        // (every one of its P x 16 workgroups — 156 KB of LDS each: one per CU — has to be RESIDENT: they wait for each other's flags.
        //  On a device with fewer CUs, a CU-masked or partitioned one, the row-chunk kernels take the engine instead)
        // h.solo = workgroups per learner: 16 (one 16-row tile each) up to 16 learners; 8 (two tiles each, a slab per tile) up to 32
        // learners — populations the row-chunk kernels used to take at 150-160 us per learn() (kernels_solo.hip has the numbers;
        // FRL_SOLO_MAXP: the largest population on this family, default 32)
        const int solo_maxp = std::min(env_int("FRL_SOLO_MAXP", 2 * kSoloMaxP), 2 * kSoloMaxP);
        int wgs = 0;
        for (int cand : {16, 8})
            if (wgs == 0 && (long long)h.P * cand <= e->n_cus && h.P * cand <= kSoloMaxP * kSoloWG) wgs = cand;
        const bool solo_fits = wgs > 0 && h.P <= solo_maxp && e->lds_per_cu >= kLdsSolo;
        h.solo = env_flag("FRL_SOLO", !named) && solo_fits ? wgs : 0;
        if (h.solo || env_flag("FRL_CRITIC_V2", h.P > 128)) h.net[0].frag = h.net[1].frag = 1;
        return h.solo ? FAM_SOLO : h.net[0].frag ? FAM_CHAINED : FAM_ROWCHUNK;
    }
    if (!wide_shape(h)) return FAM_ROWCHUNK;
    // the K-sliced chained family (kernels_criticw.hip / kernels_actorw.hip): one workgroup per (learner, agent)
    const bool named = env_set("FRL_CRITIC_V2");
    // a handful of single-agent learners at hidden 128: sixteen workgroups per learner, W1 streamed from the block (kernels_solow.hip;
    // FRL_SOLOW=0/1 overrides, FRL_CRITIC_V2 set means the caller asked for one of the other two families by name).  Every one of
    // the P x 16 workgroups has to be resident, as for kernels_solo.hip.  [s | a] must be the record's first columns, 16-byte aligned
    // ... MADDPG / MATD3 (config 5: three agents, batches of 1024): a unit = (learner, agent), 64 row tiles = 64 workgroups per unit; the
    // updating agent's own observation rows sit behind the joint rows in LDS, so both first layers have at most kSoloWActorBase k-tiles
    bool solow_shape = h.hidden == 128 && h.batch_max <= (h.n_agents == 1 ? 256 : 1024) && h.rec.stride % 4 == 0 && h.rec.obs_off[0] % 4 == 0 &&
                       h.rec.act_off[0] == h.rec.obs_off[0] + h.rec.obs_total;
    for (int i = 0; i < h.n_nets; ++i) solow_shape = solow_shape && h.net[i].L[0].k_pad <= 16 * (h.n_agents == 1 ? kSoloWMaxKB : kSoloWActorBase);
    const int solow_tiles = h.batch_max <= 256 ? kSoloWG : 4 * kSoloWG;
    const long long solow_units = (long long)h.P * h.n_agents;
    // (two row tiles per workgroup for 17 .. 32 units: measured level with the row-chunk chain — kernels_solow.hip — and not built)
    const int solow_rw = solow_tiles;
    const bool solow_fits = solow_units <= kSoloMaxP && solow_units * solow_rw <= e->n_cus && e->lds_per_cu >= kLdsSolow + 256;
    if (env_flag("FRL_SOLOW", !named) && solow_shape && solow_fits) {
        for (int i = 0; i < h.n_nets; ++i) h.net[i].frag = 1;
        h.solow = solow_tiles;
        e->solow_row_wgs = solow_rw;
        return FAM_SOLOW;
    }
    // from 129 (learner, agent) units up: hidden 128 (chain_wide.hpp) SAC at Humanoid dims 85.5 TFLOP/s against the row-chunk
    // kernels' 46.2, MADDPG simple_spread 77.2 / 55.5; hidden 256 (chain_wide16.hpp: x-stationary sweeps) 71.1 / 56.9
    // (profiles/r04, DESIGN.md 8)
    // (profiles/r04/family_crossover.txt: hidden 128 ties at ~110-129 units; hidden 256 at 128 units 38.9 against 53.1, at 192
    // 55.3 / 51.5, at 256 68.0 / 55.7 — its workgroups are twice as long, so the half-empty chip costs more: from 177 up)
    if (!env_flag("FRL_CRITIC_V2", (long long)h.P * h.n_agents > (h.hidden == 256 ? 176 : 128))) return FAM_ROWCHUNK;
    for (int i = 0; i < h.n_nets; ++i) h.net[i].frag = 1;
    h.wide = h.hidden == 256 ? 2 : 1;
    h.wide_bm = h.wide == 2 ? (h.batch_max + 255) / 256 * 256 : (h.batch_max + 63) / 64 * 64;      // (hidden 256 works in super-chunks of 256 rows)
    h.wide_xp = h.net[1].L[0].k_pad;
    h.wide_op = 16;
    for (int j = 0; j < h.n_agents; ++j) h.wide_op = std::max(h.wide_op, h.net[2 * j].L[0].k_pad);
    h.wide_unit = ((h.wide_xp + h.n_agents * h.wide_op + (h.wide == 2 ? kWide16ScratchPerRowHost : kWideScratchPerRow)) * h.wide_bm + 128 + 63) / 64 * 64;
    return h.wide == 2 ? FAM_WIDE16 : FAM_WIDE;
}

// The family THIS call runs: Batch_ObsNorm can be switched on after create and FRL_DQN_FUSED=0/1 is a per-call override.  The narrow
// families take batches of up to 256 rows; the others any batch <= batch_max (super-chunks of 256 rows / a 16-row tile per workgroup).
static LearnFamily learn_family(const frl_engine* e, int batch) {
    const EngineDesc& h = e->h;
    if (dqn_fused_shape(h, batch) && env_flag("FRL_DQN_FUSED", true)) return FAM_DQN_FUSED;
    const bool narrow = e->family == FAM_CHAINED || e->family == FAM_SOLO;
    return (h.obs_norm_on || (narrow && batch > 256)) ? FAM_ROWCHUNK : e->family;
}

// workgroups per learner of the one-launch DQN update (kernels_dqn2.hip).  A few learners: one 64-row chunk per workgroup (the
// last to arrive reduces and steps); populations: one workgroup each (measured: P = 64 x 4 workgroups 74 us, x 1 45 us).
static int dqn_split_for(const EngineDesc& h, int batch, int pc) {
    const int nchunks = (batch + 63) / 64;
    int split = (pc <= 16) ? std::min(std::min(4, nchunks), h.S) : 1;
    if (env_set("FRL_DQN_SPLIT")) split = std::max(1, std::min(std::min(env_int("FRL_DQN_SPLIT", 0), nchunks), h.S));
    return split;
}

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
    const LearnFamily fam = learn_family(e, batch);
    int bytes = e->kern.lds_bytes, rows = batch;
    switch (fam) {
        case FAM_ROWCHUNK: bytes = e->lds_bytes; rows = h.rc; break;
        case FAM_DQN_FUSED: { const int sp = dqn_split_for(h, batch, h.P); rows = std::min(((batch + 63) / 64 + sp - 1) / sp * 64, batch); break; }
        // kernels_solo.hip: 16-row tiles, 16 / h.solo of them per workgroup (its own carve; the launch carries the rollout tail's on top)
        case FAM_SOLO: bytes = solo_lds_floats() * (int)sizeof(float); rows = 16 * (kSoloWG / h.solo); break;
        case FAM_SOLOW: rows = 16 * (h.solow / std::max(1, e->solow_row_wgs)); break;      // one 16-row tile per workgroup
        default: break;                                                                      // one workgroup per unit walks the batch
    }
    if (chained_out) *chained_out = fam != FAM_ROWCHUNK;
    if (bytes_out) *bytes_out = bytes;
    if (rows_out) *rows_out = rows;
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

// the row-chunk kernels: a gradient launch over (unit, slab) workgroups, then reduce + clip + Adam
static void launch_rowchunk(frl_engine* e, const LearnStage& s, const LearnArgs& a) {
    const EngineDesc& h = e->h;
    const bool actor = s.stage == 1, sac = h.algo == ALGO_SAC || h.algo == ALGO_SAC_DISCRETE, maddpg = h.algo == ALGO_MADDPG;
    const int ns = ((a.batch + h.rc - 1) / h.rc + h.cps - 1) / h.cps;      // workgroups (= slabs) per unit
    const dim3 grid_chunks(((s.units + 7) / 8) * 8 * ns), grid_adam(s.units * h.Gmax);
    auto k = actor ? (h.algo == ALGO_SAC_DISCRETE ? sacd_actor_kernel : ac_actor_kernel)
                   : (h.algo == ALGO_DQN ? (h.c51_atoms ? c51_grad_kernel : dqn_grad_kernel) : h.algo == ALGO_SAC_DISCRETE ? sacd_critic_kernel : ac_critic_kernel);
    prof_begin(e, actor ? PK_GRAD_ACTOR : PK_GRAD_CRITIC);
    hipLaunchKernelGGL(k, grid_chunks, dim3(256), e->lds_bytes, s.st, e->d, a, ns);
    prof_end(e);
    AdamArgs ad{};
    ad.ns = ns; ad.batch = a.batch; ad.eps = a.adam_eps; ad.beta1 = a.beta1; ad.beta2 = a.beta2; ad.clip = a.clip_norm;
    ad.tau = a.tau; ad.alpha_lr = a.alpha_lr; ad.target_entropy = a.target_entropy; ad.p0 = s.p0; ad.G = h.Gmax;
    if (actor) {
        ad.which = 1; ad.lr = a.actor_lr; ad.wd = 0.f; ad.soft = maddpg ? 0 : 1; ad.sac_alpha = sac ? 1 : 0;
    } else {
        ad.which = 0; ad.lr = a.critic_lr; ad.wd = a.critic_wd;
        ad.soft = (h.algo == ALGO_DQN) ? 1 : ((!maddpg && a.do_actor) ? 1 : 0);
    }
    prof_begin(e, actor ? PK_ADAM_ACTOR : PK_ADAM_CRITIC);
    launch_adam(e, s.st, ad, s.units, grid_adam);      // (a NoisyLinear head's sigma gradients are derived in its slab sums)
    prof_end(e);
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
        case FAM_ROWCHUNK: launch_rowchunk(e, s, a); break;
        case FAM_CHAINED: launch_chained(e, s, a); break;
        case FAM_SOLO: launch_solo(e, s, a, sstep); break;
        case FAM_SOLOW: launch_solow(e, s, a, ma_predraw, ma_use_pre); break;
        case FAM_WIDE: case FAM_WIDE16: launch_wide(e, s, a); break;
        case FAM_DQN_FUSED: break;
    }
}

// `step` (frl_rollout only, DQN engines on the fused path): the vector step's add() and the next select_action in the same launch
// size_override >= 0: the rings' common size WHEN THE LAUNCH RUNS (a pre-armed launch of frl_rollout is enqueued before the step's rows
// are counted in e->size)
static int learn_impl(frl_engine* e, const frl_learn_args* args, const DqnStepArgs* step, const SoloStepArgs* sstep = nullptr, int size_override = -1,
                      hipStream_t stream_override = nullptr) {
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
    const bool td3_like = (h.algo == ALGO_TD3 || h.algo == ALGO_MADDPG);       // MADDPG + noise/delay = MATD3_simple.py
    const bool needs_noise = (h.algo == ALGO_SAC) || (td3_like && args->use_policy_noise);
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
    const bool actor_stage = (h.algo != ALGO_DQN && a.do_actor), soft_stage = (h.algo == ALGO_MADDPG && a.do_actor && fam != FAM_SOLOW);
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
    if (actor_stage && !a.fuse_actor) launch_learn_stage(e, lst, fam, a, 1, 0, h.P, dev_rng, needs_noise, nullptr, sstep ? &s1 : nullptr);
    if (soft_stage) launch_learn_stage(e, lst, fam, a, 2, 0, h.P, dev_rng, needs_noise);
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
