// What frl_create decides about an engine before it allocates anything: which configurations are refused, the nets and the record,
// the kernel family of frl_learn, LDS bytes, row chunk and every buffer size.  Arithmetic on frl_config alone — plain C++17, no HIP,
// no getenv — so tests/engine_plan_probe.cpp runs the whole create-time matrix on the CPU (tests/test_engine_plan.py).
// frl_api.hip reads the device's limits and the create-time knobs, calls plan_engine and allocates what the plan says.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/freerl_hip.h"
#include "frl_desc.h"
#include "rowchunk_layout.h"
#include "actor_park_layout.h"

namespace frl {

inline int pad16(int x) { return (x + 15) / 16 * 16; }
inline int pad32(int x) { return (x + 31) / 32 * 32; }

// What the host API needs to know about an algorithm beyond its nets: one row per frl_algo, read through algo_traits().  A new algorithm
// is a row here, its case in each of plan_engine's three steps and its own learn entry point (DESIGN.md "Where an algorithm is
// registered on the host").
inline constexpr char kFrlLearn[] = "frl_learn";
struct AlgoTraits {
    const char* name;          // in messages
    const char* learn;         // the entry point that updates such an engine ("": none)
    const char* act_hint;      // how to act when frl_act_explore (and with it frl_rollout's collection) does not serve the engine; "": it does
    bool index_action;         // the record holds the action as one index column whatever frl_config.discrete says
    bool discrete_head;        // n_discrete = act_dim[0]
    bool vector_reward;        // reward_dim reward columns, the preference buffers (env_w), batch_max counting batch x weight_num rows
    bool two_wg;               // row chunks at two workgroups per CU: hidden <= 256, <= 80 KB of LDS per chunk, no bump from 16 to 32 rows
    bool row_walks_head;       // one thread per row walks the head's act_dim x reward_dim columns: at most kSacdMaxActions of them
    bool act_spill;            // the actor stage parks activations in act_spill
    bool rollout;              // frl_rollout collects for it
};
inline constexpr AlgoTraits kAlgo[] = {
    // name            learn                      act_hint                                                                        index  disc   vecrew two_wg walks  spill  rollout
    {"replay-only",    "",                        "",                                                                             false, false, false, false, false, false, false},
    {"DQN",            kFrlLearn,                 "",                                                                             false, true,  false, false, false, false, true},
    {"DDPG",           kFrlLearn,                 "",                                                                             false, false, false, false, false, true,  true},
    {"TD3",            kFrlLearn,                 "",                                                                             false, false, false, false, false, true,  true},
    {"SAC",            kFrlLearn,                 "",                                                                             false, false, false, false, false, true,  true},
    {"MADDPG",         kFrlLearn,                 "",                                                                             false, false, false, false, false, true,  false},
    {"PPO",            "frl_ppo_learn",           "",                                                                             false, false, false, false, false, false, false},
    {"discrete SAC",   kFrlLearn,                 "FRL_ACT_CAT_SAMPLE / FRL_ACT_ARGMAX",                                          true,  true,  false, true,  true,  false, false},
    {"REINFORCE",      "frl_reinforce_learn",     "FRL_ACT_CAT_SAMPLE / FRL_ACT_ARGMAX",                                          true,  true,  false, true,  true,  false, false},
    {"envelope DQN",   "frl_envelope_learn",      "FRL_ACT_RAW on [obs | preference]; the caller weighs the objectives",          true,  true,  true,  true,  true,  false, false},
    {"envelope DDPG",  "frl_envelope_ddpg_learn", "FRL_ACT_TANHHEAD on net 0 with [obs | preference]",                            false, false, true,  true,  false, true,  false},
    {"GAIL",           "frl_gail_learn",          "FRL_ACT_RAW on [obs | act]: the discriminator's logits; rewards: frl_gail_reward",   false, false, false, true,  false, false, false},
    {"MAPPO",          "frl_mappo_learn",         "FRL_ACT_PPO_SAMPLE / FRL_ACT_CAT_SAMPLE on net 2i with agent i's observation",  false, false, false, false, false, false, false},
    {"IPPO",           "frl_mappo_learn",         "FRL_ACT_PPO_SAMPLE / FRL_ACT_CAT_SAMPLE on net 2i with agent i's observation",  false, false, false, false, false, false, false},
    {"HAPPO",          "frl_happo_learn",         "FRL_ACT_PPO_SAMPLE / FRL_ACT_CAT_SAMPLE on net 2i with agent i's observation",  false, false, false, false, false, false, false},
    {"ATT-MADDPG",     kFrlLearn,                 "",                                                                             false, false, false, false, false, true,  false},
    {"MASAC",          kFrlLearn,                 "FRL_ACT_SAC_SAMPLE / FRL_ACT_TANHHEAD on net 2i with agent i's observation",   false, false, false, false, false, true,  false},
    {"GAIL-PPO",       "frl_gail_ppo_learn",      "FRL_ACT_PPO_SAMPLE / FRL_ACT_TANHHEAD / FRL_ACT_CAT_SAMPLE on net 0, FRL_ACT_RAW on net 1: the value", false, false, false, false, false, false, false},
    {"(unassigned)",   "",                        "",                                                                             false, false, false, false, false, false, false},      // 17: refused as an unknown algo (check_create_args)
    {"CEM-GD3PG",      "frl_cem_gd3pg_learn",     "FRL_ACT_TANHHEAD on net 0 / 1 / 3 (actor_1 / actor_2 / actor_domain), FRL_ACT_RAW on net 2 with [obs | act]", false, false, false, false, false, true,  false},
};
constexpr int kAlgoUnassigned = 17;      // a value no frl_algo has: its kAlgo row only keeps the table indexable by value
inline bool is_maddpg(int algo) { return algo == FRL_ALGO_MADDPG || algo == FRL_ALGO_MADDPG_ATT; }       // what frl_learn steps as MADDPG_simple.learn does
// (FRL_ALGO_MASAC shares MADDPG's record, its nets 2i / 2i+1 and the frl_learn entry, but is NOT is_maddpg: it has no delayed policy step, no
//  policy noise and its own launch order — learn_impl and the launchers ask for it by name)
inline bool is_multi_agent_replay(int algo) { return is_maddpg(algo) || algo == FRL_ALGO_MASAC; }      // n_agents > 1 on a replay ring, learnt by frl_learn
inline bool is_mappo(int algo) { return algo == FRL_ALGO_MAPPO || algo == FRL_ALGO_IPPO; }                 // what frl_mappo_learn updates
inline bool is_mappo_family(int algo) { return is_mappo(algo) || algo == FRL_ALGO_HAPPO; }              // ... and what is built, and acts, like them
static_assert(sizeof kAlgo / sizeof kAlgo[0] == FRL_ALGO_CEM_GD3PG - FRL_ALGO_REPLAY_ONLY + 1, "one kAlgo row per frl_algo");
inline const AlgoTraits& algo_traits(int algo) { return kAlgo[algo - FRL_ALGO_REPLAY_ONLY]; }

// The kernel family an engine's frl_learn() runs on (frl_api_learn.inc: kLearnKernels registers each family's kernels).
// plan_engine fixes the engine's chained family — or none: FAM_ROWCHUNK — with its parameter layout; learn_family() says what one call takes.
// FAM_ATT: the attention critic's row-chunk kernels (kernels_att.hip) — what every FRL_ALGO_MADDPG_ATT engine learns with, and nothing else does
// FAM_MASAC: MASAC's row-chunk kernels (kernels_masac.hip): one critic launch, then one actor launch per agent — every FRL_ALGO_MASAC engine, nothing else
enum LearnFamily { FAM_ROWCHUNK, FAM_DQN_FUSED, FAM_CHAINED, FAM_SOLO, FAM_SOLOW, FAM_WIDE, FAM_WIDE16, FAM_ATT, FAM_MASAC };
// dynamic LDS of a family's launches = its kernels' hipFuncAttributeMaxDynamicSharedMemorySize
constexpr int kLdsDqnFused = dqn2_lds_floats() * (int)sizeof(float);
constexpr int kLdsChain4 = critic2_lds_floats() * (int)sizeof(float), kLdsChain8 = critic8_lds_floats() * (int)sizeof(float);
constexpr int kLdsSolo = std::max(solo_lds_floats(), critic2_lds_floats()) * (int)sizeof(float);      // (critic2: the rollout tail's act_frag_body)
constexpr int kLdsSolow = solow_lds_floats() * (int)sizeof(float);
constexpr int kLdsWide = wide_lds_floats() * (int)sizeof(float), kLdsWide16 = wide16_lds_floats_host() * (int)sizeof(float);
constexpr int kLdsMasac = 160 * 1024;     // ... and a FAM_MASAC launch (the row chunk is chosen for two workgroups per CU where the nets allow it)
constexpr int kLdsAtt = 160 * 1024;       // the most a FAM_ATT launch may carve; a launch carves its engine's own row-chunk bytes (plan_sizes refuses more)

struct PlanLimits {               // of the device
    int n_cus = 256;              // compute units (how many one-per-CU workgroups are resident at once)
    int lds_per_cu = 160 * 1024;  // LDS bytes of one compute unit
};
// The developer / test knobs that are read once, at create (frl_api.hip fills them from the environment: create_knobs).
// A tri-state is -1 unset, 0 or 1; knob_flag() applies its default.
struct PlanKnobs {
    int assume_cus = 0;           // FRL_ASSUME_CUS (tests: a smaller / partitioned device); > 0 replaces PlanLimits::n_cus
    int rc = 0;                   // FRL_RC: rows per workgroup (16 / 32 / 64 / 128)
    int cps = 0;                  // FRL_CPS: row chunks per gradient workgroup
    bool solow_narrow = false;    // FRL_SOLOW_NARROW=1: the narrow standard shape on kernels_solow.hip — one first-layer k-tile — for A/Bs against kernels_solo.hip
    int critic_v2 = -1;           // FRL_CRITIC_V2 (tri-state): the chained / wide family by name, whatever the population
    int solo = -1;                // FRL_SOLO (tri-state)
    int solo_maxp = 2 * kSoloMaxP;   // FRL_SOLO_MAXP: the largest population on kernels_solo.hip
    int solow = -1;               // FRL_SOLOW (tri-state)
    bool solow_helpers = true;    // FRL_SOLOW_HELPERS=0: no helper workgroups
    int chain_waves = 8;          // FRL_CHAIN_WAVES: waves per workgroup of the register-chained actor-critic kernels (4: round 5's)
    bool actor_park = true;       // FRL_ACTOR_PARK=0: the eight-wave chained actor stage recomputes its forward in pass C instead of parking pass A's activations
};
inline bool knob_flag(int tri, bool dflt) { return tri < 0 ? dflt : tri != 0; }

// What the plan fixes next to the descriptor.  frl_engine (frl_api.hip) inherits it: the plan is copied into an engine by one assignment
struct EngineFacts {
    LearnFamily family = FAM_ROWCHUNK;    // the chained kernel family the engine was created for (host only; frl_obsnorm_enable moves it to the row-chunk kernels for good)
    int lds_bytes = 0;            // of a row chunk
    bool has_nets = false;
    int noisy_per_set = 0;        // floats of device noise per (learner, forward): 2 * (k_pad + n_pad) of the head
    size_t idx_count = 0, noise_count = 0;      // ints / floats of the idx and noise uploads
    size_t slab_count = 0, part_count = 0, act_spill_count = 0;      // floats of the row-chunk kernels' slab, part and act_spill (rowchunk_layout.h; act_spill: 0 where no actor stage parks)
    size_t alpha_count = 0, steps_count = 0;    // floats of EngineDesc::alpha, ints of EngineDesc::steps (MASAC: per-agent alpha blocks and counters)
    int solo_stride = 0;          // floats per gradient slab of kernels_solo.hip / kernels_solow.hip: the largest net
    int solow_row_wgs = 0;        // kernels_solow.hip: workgroups per unit that own row tiles (16: one tile each; 64: MADDPG's batches of 1024)
    int solow_wgs = 0;            // ... workgroups per unit in its grids (row-tile workgroups + helpers for the update)
    size_t act_wk_slot = 0;       // floats per slot of select_action's Wk-layout copies = P * largest net
    int chain_waves = 8;          // waves per workgroup of the register-chained actor-critic kernels
    bool actor_park = true;       // the eight-wave chained actor stage reads pass A's activations back from EngineDesc::actor_park (false: it recomputes them)
    size_t actor_park_count = 0;  // floats of EngineDesc::actor_park (actor_park_layout.h); 0 on every engine outside the chained family
    int n_cus = 256;              // compute units of the device the plan was made for (FRL_ASSUME_CUS applied)
    int lds_per_cu = 160 * 1024;  // LDS bytes of one compute unit
    int n_rings = 1;              // replay rings per learner (CEM_GD3PG: 2, `buffer` and `buffer_domain`), side by side in EngineDesc::replay
    int ring_cap = 0;             // rows of one ring = frl_config.capacity; EngineDesc::capacity = n_rings * ring_cap rows per learner
};
// Everything the allocation step of frl_create needs: it makes no decisions of its own
struct EnginePlan : EngineFacts {
    EngineDesc h;                 // the finished descriptor, every device pointer null
};

// a refusal: FRL_ERR_INVALID and its text, cut like every message of the API (frl_api.hip: fail)
__attribute__((format(printf, 2, 3))) inline int plan_refuse(std::string* message, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (message) *message = buf;
    return FRL_ERR_INVALID;
}

// ------------------------------------------------------------------------------ descriptors
inline int build_net(NetDesc& N, const std::vector<std::pair<int, int>>& layers_in /* (out,in) */, int heads,
                     int hidden_act, int out_act, int extra_n, int n_shadow = 0) {
    memset(&N, 0, sizeof N);
    std::vector<std::pair<int, int>> layers = layers_in;
    for (int i = 0; i < n_shadow; ++i) layers.push_back(layers_in.back());       // sigma of a NoisyLinear head: same shape as the head
    N.n_layers = (int)layers.size();
    N.heads = heads;
    N.hidden_act = hidden_act;
    N.out_act = out_act;
    int off = 0, np = 0;
    for (int i = 0; i < N.n_layers; ++i) {
        LayerDesc& L = N.L[i];
        L.n = layers[i].first;
        L.k = layers[i].second;
        L.n_pad = pad16(L.n);
        L.k_pad = pad16(L.k);
        L.w_off = off;
        off += L.n_pad * L.k_pad;
        L.b_off = off;
        off += L.n_pad;
        np += L.n * L.k + L.n;
    }
    N.extra_off = -1;
    N.extra_n = extra_n;
    if (extra_n > 0) {
        N.extra_off = off;
        off += pad16(extra_n);
        np += extra_n;
    }
    N.size = pad32(off);
    N.n_params = np;
    N.n_layers -= n_shadow;
    N.n_shadow = n_shadow;
    return 0;
}

inline void build_record(RecordDesc& R, const frl_config& c) {
    memset(&R, 0, sizeof R);
    R.n_agents = c.n_agents;
    const AlgoTraits& T = algo_traits(c.algo);
    int off = 0;
    for (int j = 0; j < c.n_agents; ++j) { R.obs_off[j] = off; R.obs_dim[j] = c.obs_dim[j]; off += c.obs_dim[j]; }
    R.obs_total = off;
    for (int j = 0; j < c.n_agents; ++j) {
        R.act_off[j] = off;
        R.act_dim[j] = (c.discrete || T.index_action) ? 1 : c.act_dim[j];
        off += R.act_dim[j];
    }
    R.act_total = off - R.obs_total;
    R.rew_off = off; off += T.vector_reward ? std::max(1, c.reward_dim) : c.n_agents;
    R.done_off = off; off += c.n_agents;
    for (int j = 0; j < c.n_agents; ++j) { R.nobs_off[j] = off; off += c.obs_dim[j]; }
    R.extra_off = off;
    R.extra = c.extra_cols;
    off += c.extra_cols;
    R.width = off;
    R.stride = pad32(off);
}

// what frl_record_layout_get reports
inline void record_layout(const RecordDesc& R, frl_record_layout* out) {
    memset(out, 0, sizeof *out);
    out->n_agents = R.n_agents;
    out->width = R.width;
    out->stride = R.stride;
    for (int j = 0; j < R.n_agents; ++j) {
        out->obs_off[j] = R.obs_off[j]; out->obs_dim[j] = R.obs_dim[j];
        out->act_off[j] = R.act_off[j]; out->act_dim[j] = R.act_dim[j];
        out->next_obs_off[j] = R.nobs_off[j];
    }
    out->rew_off = R.rew_off;
    out->done_off = R.done_off;
    out->extra_off = R.extra_off;
    out->extra = R.extra;
}

inline int lds_bytes_for(const EngineDesc& h, int rc) {
    const int xp = h.lds_kin_pad + 4, hp = hidden_pitch(h.hidden), op = h.lds_out_pad + 4, ap = h.lds_act_pad;
    long long fl = (long long)rc * (xp + h.lds_hbufs * hp + op + 2 * ap + h.lds_row_extra) + h.lds_batch_pad + 8;
    return (int)(fl * 4);
}

// ------------------------------------------------------------------------- shape predicates
// One learner per workgroup, register-chained, Adam fused (kernels_critic2.hip / kernels_actor2.hip): the reference's standard
// narrow shape at populations that give every CU a learner; everything else takes the row-chunk kernels + reduce / Adam
// launches.  The family is chosen ONCE, at frl_create (chained_shape + population, FRL_CRITIC_V2=0/1 overrides the population
// threshold — the tests run both families on the same inputs): the chained kernels keep the nets in fragment-image order in
// HBM (NetDesc::frag), which the row-chunk kernels do not read.
inline bool chained_shape(const EngineDesc& h) {
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
inline bool wide_shape(const EngineDesc& h) {
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
inline bool dqn_fused_shape(const EngineDesc& h, int batch) {
    const NetDesc& N = h.net[0];
    return h.algo == ALGO_DQN && !h.noisy && !h.c51_atoms && h.hidden == 128 && N.n_layers == 2 &&
           N.L[0].k_pad == 16 && N.L[1].n_pad == 16 && batch <= kDqn2Batch && !h.obs_norm_on && N.hidden_act == ACT_RELU;
}

// ------------------------------------------------------------------------- family selection
// The chained family of the engine (and with it the parameter layout in HBM), fixed for the engine's life: sets h.solo / h.solow /
// h.wide (+ its scratch geometry), NetDesc::frag and solow_row_wgs.  FAM_ROWCHUNK: none.
inline LearnFamily choose_engine_family(EnginePlan& pl, const PlanKnobs& knobs) {
    EngineDesc& h = pl.h;
    const int n_cus = pl.n_cus, lds_per_cu = pl.lds_per_cu;
    if (!pl.has_nets) return FAM_ROWCHUNK;
    if (h.algo == ALGO_MASAC) return FAM_MASAC;         // (nor the stacked [mean | log_std] head, the all-actors actor loss or the per-agent launches)
    if (h.algo == ALGO_MADDPG_ATT) return FAM_ATT;      // (no chained, solo, solow or wide kernel knows the attention critic: the shapes below never see it)
    const bool named = knobs.critic_v2 >= 0;
    if (chained_shape(h) && !knobs.solow_narrow) {
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
        const int solo_maxp = std::min(knobs.solo_maxp, 2 * kSoloMaxP);
        int wgs = 0;
        for (int cand : {16, 8})
            if (wgs == 0 && (long long)h.P * cand <= n_cus && h.P * cand <= kSoloMaxP * kSoloWG) wgs = cand;
        const bool solo_fits = wgs > 0 && h.P <= solo_maxp && lds_per_cu >= kLdsSolo;
        h.solo = knob_flag(knobs.solo, !named) && solo_fits ? wgs : 0;
        if (h.solo || knob_flag(knobs.critic_v2, h.P > 128)) h.net[0].frag = h.net[1].frag = 1;
        return h.solo ? FAM_SOLO : h.net[0].frag ? FAM_CHAINED : FAM_ROWCHUNK;
    }
    if (!wide_shape(h)) return FAM_ROWCHUNK;
    // the K-sliced chained family (kernels_criticw.hip / kernels_actorw.hip): one workgroup per (learner, agent)
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
    const bool solow_fits = solow_units <= kSoloMaxP && solow_units * solow_rw <= n_cus && lds_per_cu >= kLdsSolow + 256;
    if (knob_flag(knobs.solow, !named) && solow_shape && solow_fits) {
        for (int i = 0; i < h.n_nets; ++i) h.net[i].frag = 1;
        h.solow = solow_tiles;
        pl.solow_row_wgs = solow_rw;
        return FAM_SOLOW;
    }
    // from 129 (learner, agent) units up: hidden 128 (chain_wide.hpp) SAC at Humanoid dims 85.5 TFLOP/s against the row-chunk
    // kernels' 46.2, MADDPG simple_spread 77.2 / 55.5; hidden 256 (chain_wide16.hpp: x-stationary sweeps) 71.1 / 56.9
    // (profiles/r04)
    // (profiles/r04/family_crossover.txt: hidden 128 ties at ~110-129 units; hidden 256 at 128 units 38.9 against 53.1, at 192
    // 55.3 / 51.5, at 256 68.0 / 55.7 — its workgroups are twice as long, so the half-empty chip costs more: from 177 up)
    if (!knob_flag(knobs.critic_v2, (long long)h.P * h.n_agents > (h.hidden == 256 ? 176 : 128))) return FAM_ROWCHUNK;
    for (int i = 0; i < h.n_nets; ++i) h.net[i].frag = 1;
    h.wide = h.hidden == 256 ? 2 : 1;
    h.wide_bm = h.wide == 2 ? (h.batch_max + 255) / 256 * 256 : (h.batch_max + 63) / 64 * 64;      // (hidden 256 works in super-chunks of 256 rows)
    h.wide_xp = h.net[1].L[0].k_pad;
    h.wide_op = 16;
    for (int j = 0; j < h.n_agents; ++j) h.wide_op = std::max(h.wide_op, h.net[2 * j].L[0].k_pad);
    h.wide_unit = ((h.wide_xp + h.n_agents * h.wide_op + (h.wide == 2 ? kWide16ScratchPerRowHost : kWideScratchPerRow)) * h.wide_bm + 128 + 63) / 64 * 64;
    return h.wide == 2 ? FAM_WIDE16 : FAM_WIDE;
}

// The family ONE call runs on an engine created for `family`: Batch_ObsNorm can be switched on after create and FRL_DQN_FUSED=0/1
// (dqn_fused_on) is a per-call override.  The narrow families take batches of up to 256 rows; the others any batch <= batch_max
// (super-chunks of 256 rows / a 16-row tile per workgroup).
inline LearnFamily learn_family(const EngineDesc& h, LearnFamily family, int batch, bool dqn_fused_on) {
    if (dqn_fused_shape(h, batch) && dqn_fused_on) return FAM_DQN_FUSED;
    if (family == FAM_ATT || family == FAM_MASAC) return family;
    const bool narrow = family == FAM_CHAINED || family == FAM_SOLO;
    return (h.obs_norm_on || (narrow && batch > 256)) ? FAM_ROWCHUNK : family;
}

// workgroups per learner of the one-launch DQN update (kernels_dqn2.hip).  A few learners: one 64-row chunk per workgroup (the
// last to arrive reduces and steps); populations: one workgroup each (measured: P = 64 x 4 workgroups 74 us, x 1 45 us).
// split_knob: FRL_DQN_SPLIT, read per call (< 0: unset)
inline int dqn_split_for(const EngineDesc& h, int batch, int pc, int split_knob) {
    const int nchunks = (batch + 63) / 64;
    int split = (pc <= 16) ? std::min(std::min(4, nchunks), h.S) : 1;
    if (split_knob >= 0) split = std::max(1, std::min(std::min(split_knob, nchunks), h.S));
    return split;
}

// dynamic LDS of the launches of `fam` (FAM_ROWCHUNK: the engine's own row-chunk bytes, not a constant)
inline int family_lds_bytes(LearnFamily fam, int chain_waves) {
    switch (fam) {
        case FAM_DQN_FUSED: return kLdsDqnFused;
        case FAM_CHAINED: return chain_waves == 4 ? kLdsChain4 : kLdsChain8;
        case FAM_SOLO: return kLdsSolo;
        case FAM_SOLOW: return kLdsSolow;
        case FAM_WIDE: return kLdsWide;
        case FAM_WIDE16: return kLdsWide16;
        case FAM_ATT: return kLdsAtt;
        case FAM_MASAC: return kLdsMasac;
        case FAM_ROWCHUNK: break;
    }
    return 0;
}

// what frl_learn_path reports for a call that runs on `fam` (learn_family) with dqn_split workgroups per learner (dqn_split_for)
struct LearnPath { bool chained; int bytes, rows; };
inline LearnPath learn_path(const EngineDesc& h, const EngineFacts& f, LearnFamily fam, int batch, int dqn_split) {
    int bytes = family_lds_bytes(fam, f.chain_waves), rows = batch;
    switch (fam) {
        case FAM_ROWCHUNK: case FAM_ATT: case FAM_MASAC: bytes = f.lds_bytes; rows = h.rc; break;      // (FAM_ATT: row chunks too, its own carve behind the common one)
        case FAM_DQN_FUSED: rows = std::min(((batch + 63) / 64 + dqn_split - 1) / dqn_split * 64, batch); break;
        // kernels_solo.hip: 16-row tiles, 16 / h.solo of them per workgroup (its own carve; the launch carries the rollout tail's on top)
        case FAM_SOLO: bytes = solo_lds_floats() * (int)sizeof(float); rows = 16 * (kSoloWG / h.solo); break;
        case FAM_SOLOW: rows = 16 * (h.solow / std::max(1, f.solow_row_wgs)); break;      // one 16-row tile per workgroup
        default: break;                                                                 // one workgroup per unit walks the batch
    }
    return {fam != FAM_ROWCHUNK && fam != FAM_ATT && fam != FAM_MASAC, bytes, rows};
}

// ------------------------------------------------------------------------------- the plan
// What frl_create_ex checks before it looks for a device, in this order (the messages come before "no HIP device")
inline int check_create_args(const frl_config& c, const frl_config_ext* ext, std::string* message) {
    int state_dim = 0;
    if (ext) {
        if (ext->size != (int)sizeof(frl_config_ext)) return plan_refuse(message, "frl_config_ext.size %d != sizeof(frl_config_ext) %d", ext->size, (int)sizeof(frl_config_ext));
        if (ext->state_dim < 0) return plan_refuse(message, "frl_config_ext.state_dim %d must be >= 0", ext->state_dim);
        if (ext->state_rows != FRL_STATE_ROWS_POSITION && ext->state_rows != FRL_STATE_ROWS_SAMPLE)
            return plan_refuse(message, "frl_config_ext.state_rows %d (FRL_STATE_ROWS_POSITION or FRL_STATE_ROWS_SAMPLE)", ext->state_rows);
        state_dim = ext->state_dim;
    }
    if (state_dim > 0 && c.algo != FRL_ALGO_MAPPO)
        return plan_refuse(message, "state_dim %d: a global-state critic belongs to FRL_ALGO_MAPPO engines (MAPPO_for_mask_action_state.py); algo %d has none", state_dim, c.algo);
    if (c.n_learners < 1) return plan_refuse(message, "n_learners must be >= 1");
    if (c.n_agents < 1 || c.n_agents > FRL_MAX_AGENTS) return plan_refuse(message, "n_agents out of range");
    if (!is_multi_agent_replay(c.algo) && !is_mappo_family(c.algo) && c.n_agents != 1) return plan_refuse(message, "n_agents > 1 needs FRL_ALGO_MADDPG");
    if (c.capacity < 1) return plan_refuse(message, "capacity must be >= 1");
    if (c.algo < FRL_ALGO_REPLAY_ONLY || c.algo > FRL_ALGO_CEM_GD3PG || c.algo == kAlgoUnassigned) return plan_refuse(message, "unknown algo %d", c.algo);
    for (int j = 0; j < c.n_agents; ++j)
        if (c.obs_dim[j] < 1 || c.act_dim[j] < 1) return plan_refuse(message, "obs_dim/act_dim must be >= 1");
    return FRL_OK;
}

// Step 1: what an algorithm's kernels cannot handle, as far as the configuration alone shows it (what does not fit LDS: step 3).
// h: the fields plan_engine has filled from the configuration (hidden, reward_dim)
inline int plan_refusals(const frl_config& c, int state_dim, const EngineDesc& h, std::string* message) {
    const AlgoTraits& T = algo_traits(c.algo);
    if (h.hidden % 16) return plan_refuse(message, "hidden must be a multiple of 16");
    if (T.vector_reward && c.reward_dim < 0) return plan_refuse(message, "%s: reward_dim %d must be >= 1 (0 means 1)", T.name, c.reward_dim);
    // what the kernels of these algorithms handle: one thread per row walks the head's columns; the row-chunk layout at two workgroups per CU
    if (T.row_walks_head && (long long)c.act_dim[0] * h.reward_dim > kSacdMaxActions)
        return plan_refuse(message, "%s: %d actions x %d reward columns > %d head columns", T.name, c.act_dim[0], h.reward_dim, kSacdMaxActions);
    if (T.two_wg && h.hidden > 256) return plan_refuse(message, "%s: hidden %d > 256 does not fit the row-chunk layout at two workgroups per CU", T.name, h.hidden);
    auto no_leaky_relu = [&] {
        return c.hidden_act != FRL_ACT_LEAKY_RELU ? (int)FRL_OK
               : plan_refuse(message, "FRL_ACT_LEAKY_RELU is the GAIL discriminator's hidden activation; %s engines do not take it", T.name);
    };
    switch (c.algo) {
        case FRL_ALGO_MAPPO: case FRL_ALGO_IPPO: case FRL_ALGO_HAPPO: {
            // what kernels_mappo.hip handles (the LayerNorm mask is 256 bits per row; one thread per row walks a discrete head)
            int amax = 0, lp_cols = 0;
            for (int j = 0; j < c.n_agents; ++j) { amax = std::max(amax, c.act_dim[j]); lp_cols += c.discrete ? 1 : c.act_dim[j]; }
            if (h.hidden > 256) return plan_refuse(message, "%s: hidden %d > 256 does not fit the row-chunk layout with LayerNorm", T.name, h.hidden);
            if (c.discrete && amax > kSacdMaxActions) return plan_refuse(message, "%s: %d actions > %d head columns", T.name, amax, kSacdMaxActions);
            if (c.hidden_act != FRL_ACT_RELU) return plan_refuse(message, "%s: hidden_act %d is refused (FRL_ACT_RELU: the reference's nets have no other)", T.name, c.hidden_act);
            if (c.twin_critic || c.dueling || c.noisy || c.c51_atoms || c.actor_dist != 0)
                return plan_refuse(message, "%s: twin_critic, dueling, noisy, c51_atoms and actor_dist must be 0", T.name);
            // (a discrete FRL_ALGO_MAPPO engine may carry one mask block of act_dim[i] columns per agent behind them: frl_action_mask_set)
            int mask_cols = 0;
            for (int j = 0; j < c.n_agents; ++j) mask_cols += c.act_dim[j];
            const bool with_masks = c.algo == FRL_ALGO_MAPPO && c.discrete && c.extra_cols == lp_cols + c.n_agents + mask_cols + state_dim;
            if (state_dim > 0 && c.extra_cols != lp_cols + c.n_agents + state_dim && !with_masks)      // (the state block: the last state_dim columns)
                return plan_refuse(message, "%s: extra_cols %d != %d log-prob columns + %d adv_done columns [+ %d mask columns] + %d state columns", T.name, c.extra_cols,
                                   lp_cols, c.n_agents, mask_cols, state_dim);
            if (c.extra_cols != lp_cols + c.n_agents + state_dim && !with_masks)
                return plan_refuse(message, "%s: extra_cols %d != %d log-prob columns + %d adv_done columns", T.name, c.extra_cols, lp_cols, c.n_agents);
            return FRL_OK;      // (its hidden_act rule has covered FRL_ACT_LEAKY_RELU)
        }
        case FRL_ALGO_MADDPG_ATT:
            // what kernels_att.hip handles (ATT.py:181-229: the decoder reads the OTHER agents' actions; Critic_TD3 has no attention form)
            if (c.n_agents < 2) return plan_refuse(message, "%s: n_agents %d < 2: the decoder's input is the other agents' actions and would be empty", T.name, c.n_agents);
            if (c.twin_critic) return plan_refuse(message, "%s: twin_critic is refused (the attention critic has one Q head; MATD3 keeps the plain critic)", T.name);
            if (c.discrete) return plan_refuse(message, "%s: discrete is refused (continuous actions only, as MADDPG_simple_with_tricks.py:139-144)", T.name);
            if (c.dueling || c.noisy || c.c51_atoms || c.actor_dist != 0) return plan_refuse(message, "%s: dueling, noisy, c51_atoms and actor_dist must be 0", T.name);
            if (c.hidden_act != FRL_ACT_RELU) return plan_refuse(message, "%s: hidden_act %d is refused (FRL_ACT_RELU: the reference's nets have no other)", T.name, c.hidden_act);
            if (h.hidden % 16 || h.hidden > 128)
                return plan_refuse(message, "%s: hidden %d is refused: the row chunk's 16 rows of x_e, x_d, e, g, the %d heads, d, u, c and y fit a CU's LDS up to hidden 128", T.name, h.hidden, kAttHeads);
            return FRL_OK;
        case FRL_ALGO_MASAC:
            // what kernels_masac.hip handles (MASAC.py:32-97: ReLU nets, a twin critic in one net, tanh-Gaussian actors)
            if (c.discrete)
                return plan_refuse(message, "%s: discrete is refused (continuous actions only: the reference's discrete branch calls Agent.argmax, which does not exist, MASAC.py:185)", T.name);
            if (!c.twin_critic) return plan_refuse(message, "%s: twin_critic = 0 is refused (Critic holds Q1 and Q2 in one net and the update takes their minimum, MASAC.py:72-97)", T.name);
            if (c.dueling || c.noisy || c.c51_atoms || c.actor_dist != 0) return plan_refuse(message, "%s: dueling, noisy, c51_atoms and actor_dist must be 0", T.name);
            if (c.hidden_act != FRL_ACT_RELU) return plan_refuse(message, "%s: hidden_act %d is refused (FRL_ACT_RELU: the reference's nets have no other)", T.name, c.hidden_act);
            return FRL_OK;
        case FRL_ALGO_GAIL:     // (the gradient penalty's closed form needs a piecewise-linear activation: csrc/device/gail.hpp)
            if (c.hidden_act == FRL_ACT_TANH) return plan_refuse(message, "GAIL: hidden_act FRL_ACT_TANH is refused (FRL_ACT_LEAKY_RELU or FRL_ACT_RELU)");
            return FRL_OK;
        case FRL_ALGO_GAIL_PPO:
            // what kernels_gail_ppo.hip handles (GAIL_file/PPO2.py:20-79: two 3-layer nets, LeakyReLU in GAIL's config and ReLU in PPO's own)
            if (c.hidden_act == FRL_ACT_TANH) return plan_refuse(message, "%s: hidden_act FRL_ACT_TANH is refused (FRL_ACT_LEAKY_RELU or FRL_ACT_RELU: the shipped configs have no other)", T.name);
            if (c.hidden_act != FRL_ACT_LEAKY_RELU && c.hidden_act != FRL_ACT_RELU) return plan_refuse(message, "%s: hidden_act %d is refused (FRL_ACT_LEAKY_RELU or FRL_ACT_RELU)", T.name, c.hidden_act);
            if (h.hidden > 256) return plan_refuse(message, "%s: hidden %d > 256 is refused, as for the discriminator it trains against", T.name, h.hidden);
            if (c.extra_cols != 0) return plan_refuse(message, "%s: extra_cols %d must be 0 (the old log-prob is recomputed, not stored: PPO2.py:240-250)", T.name, c.extra_cols);
            if (c.discrete && c.act_dim[0] < 2) return plan_refuse(message, "%s: a Categorical policy needs act_dim >= 2 logits", T.name);
            if (c.discrete && c.act_dim[0] > kSacdMaxActions) return plan_refuse(message, "%s: %d actions > %d head columns", T.name, c.act_dim[0], kSacdMaxActions);
            if (c.twin_critic || c.dueling || c.noisy || c.c51_atoms || c.actor_dist != 0)
                return plan_refuse(message, "%s: twin_critic, dueling, noisy, c51_atoms and actor_dist must be 0", T.name);
            return FRL_OK;
        case FRL_ALGO_CEM_GD3PG:
            // what kernels_cem_gd3pg.hip handles (CEM_GD3PG.py:30-92: tanh actors, a LeakyReLU critic with one Q head, continuous actions)
            if (c.discrete)
                return plan_refuse(message, "%s: discrete is refused (the reference builds a one-column action buffer that its critic cannot read, CEM_GD3PG.py:134)", T.name);
            if (c.twin_critic) return plan_refuse(message, "%s: twin_critic is refused (one critic serves both actors; the minimum is over the two target actors)", T.name);
            if (c.hidden_act != FRL_ACT_TANH)
                return plan_refuse(message, "%s: hidden_act %d is refused (FRL_ACT_TANH, the actors' activation; the critic is always LeakyReLU)", T.name, c.hidden_act);
            if (c.dueling || c.noisy || c.c51_atoms || c.actor_dist != 0 || c.extra_cols != 0)
                return plan_refuse(message, "%s: dueling, noisy, c51_atoms, actor_dist and extra_cols must be 0", T.name);
            if (c.capacity > (1 << 30)) return plan_refuse(message, "%s: capacity %d > 2^30 (a learner's two rings are indexed as one)", T.name, c.capacity);
            return FRL_OK;
        case FRL_ALGO_DQN:
            if (const int rc = no_leaky_relu()) return rc;
            if (c.c51_atoms > 64) return plan_refuse(message, "c51_atoms %d: the distribution arithmetic runs one wave lane per atom (<= 64; the reference uses 51)", c.c51_atoms);
            return FRL_OK;
        default:
            return no_leaky_relu();
    }
}

// Step 2: the algorithm's nets, their places in a learner's parameter block and the widest first layer / head (lds_kin_pad, lds_out_pad)
inline void plan_nets(const frl_config& c, int state_dim, EnginePlan& pl) {
    EngineDesc& h = pl.h;
    const RecordDesc& R = h.rec;
    const int H = h.hidden;
    const int hact = c.hidden_act == FRL_ACT_TANH ? ACT_TANH : ACT_RELU;
    switch (c.algo) {
        case FRL_ALGO_REPLAY_ONLY: break;
        case FRL_ALGO_DQN: {
            h.n_nets = 1;
            h.dueling = c.dueling ? 1 : 0;
            h.noisy = c.noisy ? 1 : 0;
            h.c51_atoms = c.c51_atoms > 1 ? c.c51_atoms : 0;
            h.c51_vmin = c.c51_vmin; h.c51_vmax = c.c51_vmax;
            const int per_out = h.c51_atoms ? h.c51_atoms : 1;        // head rows: [V (per_out) ;] A (act_dim x per_out)
            build_net(h.net[0], {{H, c.obs_dim[0]}, {(c.act_dim[0] + (c.dueling ? 1 : 0)) * per_out, H}}, 1, ACT_RELU, ACT_NONE, 0,
                      c.noisy ? 1 : 0);                                                                      // MLP, DQN.py:32-45
            h.noisy_split = c.dueling ? per_out : h.net[0].L[1].n_pad;
            break;
        }
        case FRL_ALGO_SAC_DISCRETE: {
            // Actor_discrete_hands_on (SAC_add_discrete.py:137-150): O -> H -> H -> A, softmax on the head (in the kernels);
            // Critic_discrete_hands_on (:152-177): two heads l1-l3 / l4-l6 on obs only, one value per action
            h.n_nets = 2;
            const int O = c.obs_dim[0], A = c.act_dim[0];
            build_net(h.net[0], {{H, O}, {H, H}, {A, H}}, 1, ACT_RELU, ACT_NONE, 0);
            build_net(h.net[1], {{H, O}, {H, H}, {A, H}, {H, O}, {H, H}, {A, H}}, 2, ACT_RELU, ACT_NONE, 0);
            break;
        }
        case FRL_ALGO_ENVELOPE_DQN:
            h.n_nets = 1;                                                   // MLP (ENVELOPE_DQN.py:36-59): [obs | w] -> H -> H -> A x R, with a target
            build_net(h.net[0], {{H, c.obs_dim[0] + h.reward_dim}, {H, H}, {c.act_dim[0] * h.reward_dim, H}}, 1, ACT_RELU, ACT_NONE, 0);
            break;
        case FRL_ALGO_ENVELOPE_DDPG:
            // Actor (ENVELOPE_DDPG.py:40-63): [obs | w] -> H -> H -> A, tanh; Critic (:65-91): [obs | act | w] -> H -> H -> R; each with a target
            h.n_nets = 2;
            build_net(h.net[0], {{H, c.obs_dim[0] + h.reward_dim}, {H, H}, {c.act_dim[0], H}}, 1, ACT_RELU, ACT_TANH, 0);
            build_net(h.net[1], {{H, c.obs_dim[0] + c.act_dim[0] + h.reward_dim}, {H, H}, {h.reward_dim, H}}, 1, ACT_RELU, ACT_NONE, 0);
            break;
        case FRL_ALGO_GAIL:
            h.n_nets = 1;                                                   // Discriminator (GAIL.py:17-28): mlp(s_dim + a_dim, [H, H], 1), no target
            build_net(h.net[0], {{H, c.obs_dim[0] + c.act_dim[0]}, {H, H}, {1, H}}, 1, c.hidden_act == FRL_ACT_LEAKY_RELU ? ACT_LEAKY_RELU : ACT_RELU, ACT_NONE, 0);
            break;
        case FRL_ALGO_REINFORCE:
            h.n_nets = 1;                                                   // Policy_MLP (REINFORCE.py:32-46): softmax in the kernels
            build_net(h.net[0], {{H, c.obs_dim[0]}, {c.act_dim[0], H}}, 1, ACT_RELU, ACT_NONE, 0);
            break;
        case FRL_ALGO_MAPPO: case FRL_ALGO_IPPO: case FRL_ALGO_HAPPO:
            // Actor / Actor_discrete (MAPPO.py:123-186 = IPPO.py:57-116) on the agent's own observation; Critic on the global observation
            // (MAPPO.py:188-218 = HAPPO.py:196-226) or on the agent's own (IPPO.py:118-153, with the agent's own index: its class counter is a defect)
            h.n_nets = 2 * c.n_agents;
            for (int j = 0; j < c.n_agents; ++j) {
                build_net(h.net[2 * j], {{H, c.obs_dim[j]}, {H, H}, {c.act_dim[j], H}}, 1, ACT_RELU, c.discrete ? ACT_NONE : ACT_TANH, c.discrete ? 0 : c.act_dim[j]);
                // (+ the global state behind the observations: MAPPO_for_mask_action_state.py:122-127; state_dim > 0 on FRL_ALGO_MAPPO only)
                build_net(h.net[2 * j + 1], {{H, mappo_joint(c.algo) ? R.obs_total + state_dim : c.obs_dim[j]}, {H, H}, {1, H}}, 1, ACT_RELU, ACT_NONE, 0);
                if (c.discrete) h.n_discrete = std::max(h.n_discrete, c.act_dim[j]);      // (a flag to these kernels: an agent's action count is its actor's head width)
            }
            break;
        case FRL_ALGO_PPO:
            h.n_nets = 2;
            if (c.discrete) h.n_discrete = c.act_dim[0];
            if (c.discrete && c.actor_dist == 2) h.cat_logits = 1;     // PPO_file/PPO.py:78-90,176,257: raw logits into Categorical(logits=)
            if (c.discrete)     // Actor_discrete (PPO_with_tricks.py:110-121): ReLU body, softmax over n_actions logits
                build_net(h.net[0], {{H, c.obs_dim[0]}, {H, H}, {c.act_dim[0], H}}, 1, ACT_RELU, ACT_NONE, 0);
            else if (c.actor_dist == 1) {   // Actor_Beta (:120-151): alpha_layer and beta_layer share the trunk = one 2A-wide head
                build_net(h.net[0], {{H, c.obs_dim[0]}, {H, H}, {2 * c.act_dim[0], H}}, 1, hact, ACT_NONE, 0);
                h.beta_actor = 1;
            } else
                build_net(h.net[0], {{H, c.obs_dim[0]}, {H, H}, {c.act_dim[0], H}}, 1, hact, ACT_TANH, c.act_dim[0]);
            build_net(h.net[1], {{H, c.obs_dim[0]}, {H, H}, {1, H}}, 1, hact, ACT_NONE, 0);
            break;
        case FRL_ALGO_GAIL_PPO: {
            // Actor / ActorDiscrete and Critic (GAIL_file/PPO2.py:20-64): mlp(s_dim, [H, H], a_dim | 1); tanh on the mean, raw logits when discrete
            h.n_nets = 2;
            const int lact = c.hidden_act == FRL_ACT_LEAKY_RELU ? ACT_LEAKY_RELU : ACT_RELU;
            if (c.discrete) { h.n_discrete = c.act_dim[0]; h.cat_logits = 1; }
            build_net(h.net[0], {{H, c.obs_dim[0]}, {H, H}, {c.act_dim[0], H}}, 1, lact, c.discrete ? ACT_NONE : ACT_TANH, c.discrete ? 0 : c.act_dim[0]);
            build_net(h.net[1], {{H, c.obs_dim[0]}, {H, H}, {1, H}}, 1, lact, ACT_NONE, 0);
            h.log_std_min = -10.f; h.log_std_max = 2.f;      // PPO2's shipped range; frl_log_std_range_set
            break;
        }
        case FRL_ALGO_CEM_GD3PG: {
            // Actor (CEM_GD3PG.py:30-49) three times: actor_1, actor_2 and, behind the critic, the frozen actor_domain; Critic (:74-92)
            h.n_nets = 4;
            const int O = c.obs_dim[0], A = c.act_dim[0];
            for (int i : {0, 1, 3}) build_net(h.net[i], {{H, O}, {H, H}, {A, H}}, 1, ACT_TANH, ACT_TANH, 0);
            build_net(h.net[2], {{H, O + A}, {H, H}, {1, H}}, 1, ACT_LEAKY_RELU, ACT_NONE, 0);
            break;
        }
        case FRL_ALGO_MADDPG_ATT:
            // Actor (MADDPG_simple_with_tricks.py:57-69) as MADDPG's; ATT_critic (ATT.py:181-229) as the seven layers of AttLayer: the encoder
            // reads [every observation | a_i], the decoder the other agents' actions, the four heads are one layer of 4 H outputs
            h.n_nets = 2 * c.n_agents;
            for (int j = 0; j < c.n_agents; ++j) {
                build_net(h.net[2 * j], {{H, c.obs_dim[j]}, {H, H}, {c.act_dim[j], H}}, 1, ACT_RELU, ACT_TANH, 0);
                build_net(h.net[2 * j + 1], {{H, H}, {kAttHeads * H, H}, {H, H}, {H, R.obs_total + R.act_dim[j]}, {H, R.act_total - R.act_dim[j]}, {H, H}, {1, H}},
                          1, ACT_RELU, ACT_NONE, 0);
            }
            break;
        case FRL_ALGO_MASAC: {
            // Actor (MASAC.py:32-47): l1, l2 and mean_layer / log_std_layer as ONE head of 2 A outputs, rows [0, A) the mean and [A, 2 A) log_std
            // (no extra vector); Critic (:72-97): Q1 = l1, l2, l3 and Q2 = l1_2, l2_2, l3_2 on [all obs | all actions] in one net
            h.n_nets = 2 * c.n_agents;
            const int cin = R.obs_total + R.act_total;
            for (int j = 0; j < c.n_agents; ++j) {
                build_net(h.net[2 * j], {{H, c.obs_dim[j]}, {H, H}, {2 * c.act_dim[j], H}}, 1, ACT_RELU, ACT_NONE, 0);
                build_net(h.net[2 * j + 1], {{H, cin}, {H, H}, {1, H}, {H, cin}, {H, H}, {1, H}}, 2, ACT_RELU, ACT_NONE, 0);
            }
            break;
        }
        default: {      // DDPG, TD3, SAC, MADDPG: an actor and a (twin) critic on the joint [obs | act] per agent
            h.n_nets = 2 * c.n_agents;
            const int cin = R.obs_total + R.act_total;
            const int heads = c.twin_critic ? 2 : 1;
            for (int j = 0; j < c.n_agents; ++j) {
                const bool sac = c.algo == FRL_ALGO_SAC;
                build_net(h.net[2 * j], {{H, c.obs_dim[j]}, {H, H}, {c.act_dim[j], H}}, 1, ACT_RELU,
                          sac ? ACT_NONE : ACT_TANH, sac ? c.act_dim[j] : 0);
                std::vector<std::pair<int, int>> ls;
                for (int hd = 0; hd < heads; ++hd) { ls.push_back({H, cin}); ls.push_back({H, H}); ls.push_back({1, H}); }
                build_net(h.net[2 * j + 1], ls, heads, ACT_RELU, ACT_NONE, 0);
            }
            break;
        }
    }
    int off = 0, kin = 16, outp = 16;
    for (int i = 0; i < h.n_nets; ++i) {
        h.net_off[i] = off;
        off += h.net[i].size;
        const int nl = h.net[i].n_layers / h.net[i].heads;
        if (c.algo == FRL_ALGO_MADDPG_ATT && (i & 1)) {      // no chain: xin holds x_e, the first-layer input of the encoder branch
            kin = std::max(kin, h.net[i].L[ATT_E].k_pad);
            continue;
        }
        for (int hd = 0; hd < h.net[i].heads; ++hd) {
            kin = std::max(kin, h.net[i].L[hd * nl].k_pad);
            outp = std::max(outp, h.net[i].L[hd * nl + nl - 1].n_pad);
        }
    }
    h.learner_stride = pad32(off);
    h.lds_kin_pad = kin;
    h.lds_out_pad = outp;
}

// Step 3: the kernel family, the LDS carve, the row chunk (refusing what does not fit a CU's LDS), chunks per workgroup and the sizes
// of the buffers that follow from them
inline int plan_sizes(const frl_config& c, const PlanKnobs& knobs, EnginePlan& pl, std::string* message) {
    EngineDesc& h = pl.h;
    const RecordDesc& R = h.rec;
    const AlgoTraits& T = algo_traits(c.algo);
    const int H = h.hidden;
    pl.family = choose_engine_family(pl, knobs);
    pl.chain_waves = knobs.chain_waves == 4 ? 4 : 8;
    pl.actor_park = knobs.actor_park;
    h.act_max = 1;
    for (int j = 0; j < c.n_agents; ++j) h.act_max = std::max(h.act_max, R.act_dim[j]);
    // one hidden-activation buffer is enough when every head is input -> hidden -> output (DQN's Q-net): 17 KB less per 32-row
    // chunk, which puts the Categorical update's 32-row workgroups at two per CU
    h.lds_hbufs = 1;
    for (int i = 0; i < h.n_nets; ++i)
        if (h.net[i].n_layers / std::max(1, h.net[i].heads) > 2) h.lds_hbufs = 2;
    h.lds_batch_pad = 128;                                  // y holds one row chunk (rc <= 128) of TD targets
    h.lds_act_pad = (std::max(R.act_total, 1) + 3) / 4 * 4; // abuf / dabuf are scalar-accessed: no tile padding
    // projected distribution / probabilities per row, and the row's q value per action (more actions than atoms: 7 on 3 atoms)
    if (h.c51_atoms) h.lds_act_pad = std::max(h.lds_act_pad, (std::max(h.c51_atoms, c.act_dim[0]) + 3) / 4 * 4);
    if (T.vector_reward) h.lds_act_pad = std::max(h.lds_act_pad, (h.reward_dim + 3) / 4 * 4);                    // the target vector per row
    bool one_wg_per_net = false;      // a persistent kernel, one workgroup per net whatever rc is: it prefers the whole minibatch in one chunk
    bool whole_cu = false;            // ... and the largest chunk ONE workgroup's LDS holds
    int call_rows = h.batch_max;      // the most rows one learn call brings
    switch (c.algo) {
        case FRL_ALGO_PPO:
            if (c.discrete) h.lds_act_pad = std::max(h.lds_act_pad, pad16(c.act_dim[0]));   // logits' delta staging
            if (c.actor_dist == 1) h.lds_act_pad = std::max(h.lds_act_pad, pad16(2 * c.act_dim[0]));
            one_wg_per_net = true;
            break;
        case FRL_ALGO_GAIL_PPO:          // two persistent workgroups per learner, like PPO's
            if (c.discrete) h.lds_act_pad = std::max(h.lds_act_pad, pad16(c.act_dim[0]));   // logits' delta staging (continuous: act_dim columns of log_std terms)
            one_wg_per_net = true;
            break;
        case FRL_ALGO_SAC_DISCRETE:
            h.lds_act_pad = std::max(h.lds_act_pad, (c.act_dim[0] + 3) / 4 * 4);   // p' / min(Q1', Q2') per row
            break;
        case FRL_ALGO_GAIL:
            h.lds_act_pad = std::max(h.lds_act_pad, ((H + 31) / 32 + 3) / 4 * 4);             // abuf / dabuf: a row's slope bits of h1 / h2
            call_rows = 2 * h.batch_max;      // (a call has up to batch_max expert rows AND up to batch_max policy rows)
            break;
        case FRL_ALGO_MAPPO: case FRL_ALGO_IPPO: case FRL_ALGO_HAPPO:      // one persistent workgroup per (learner, agent, net), like PPO's
            if (c.discrete) h.lds_act_pad = std::max(h.lds_act_pad, h.lds_out_pad);      // logits' delta staging
            h.lds_row_extra = mappo_row_extra(H);                               // reserved for the LayerNorm case: frl_net_norm_set cannot fail for space
            one_wg_per_net = whole_cu = true;
            break;
        case FRL_ALGO_MASAC:             // device/masac.hpp: the updating actor's head row behind the common carve
            h.lds_row_extra = masac_row_extra(h.act_max);
            break;
        case FRL_ALGO_MADDPG_ATT: {      // device/att.hpp: carve_att behind the common carve
            int xd = 16;
            for (int j = 0; j < c.n_agents; ++j) xd = std::max(xd, h.net[2 * j + 1].L[ATT_D].k_pad);
            h.lds_row_extra = att_row_extra(H, xd);
            break;
        }
        default: break;
    }
    h.rc = 64;
    if (whole_cu) {
        while (h.rc > 16 && lds_bytes_for(h, h.rc) > 160 * 1024) h.rc /= 2;
    } else {
        // row chunk: the largest of {64,32,16} whose LDS footprint still lets TWO workgroups share a CU.  Measured
        // (profiles/README.md v4): 64 rows x 2 workgroups beats 32 x 3, 32 x 4 and 128 x 1 — more rows per weight fragment
        // fetched and half the gradient slabs, while two workgroups still overlap each other's barrier phases
        while (h.rc > 16 && lds_bytes_for(h, h.rc) > 80 * 1024) h.rc /= 2;   // two workgroups per CU (160 KB LDS)
        // wide inputs (SAC on Humanoid: 393 input columns): 16 rows re-read every weight 16x per batch; 32 rows at ONE
        // workgroup per CU measured +8 % over 16 rows at three (tools/config_bench.py, SAC C4)
        if (h.rc == 16 && lds_bytes_for(h, 32) <= 160 * 1024 && !T.two_wg) h.rc = 32;
        // small populations cannot fill 256 CUs with 64-row chunks (one learner = batch/64 workgroups): 32-row chunks double
        // the workgroup count and measured +19 % (P = 1) / +13 % (P = 8) updates/s
        if (!one_wg_per_net && h.rc == 64 && (long long)h.P * ((h.batch_max + 63) / 64) < 512) h.rc = 32;
    }
    if (knobs.rc == 16 || knobs.rc == 32 || knobs.rc == 64 || knobs.rc == 128) h.rc = knobs.rc;      // developer knob
    if (c.algo == FRL_ALGO_MADDPG_ATT) {      // one workgroup per CU at 16 rows: the family's row chunk is a constant (DESIGN.md "ATT-MADDPG")
        h.rc = kAttRc;
        if (lds_bytes_for(h, h.rc) > kLdsAtt)
            return plan_refuse(message, "%s: %d B of LDS per 16-row chunk > 160 KB (encoder input %d columns, decoder input at most %d)", T.name, lds_bytes_for(h, h.rc),
                               h.lds_kin_pad, h.lds_row_extra - 4 - 4 * (H + 4) - (kAttHeads * H + 4));
    }
    if (c.algo == FRL_ALGO_MASAC && lds_bytes_for(h, h.rc) > kLdsMasac)
        return plan_refuse(message, "%s: hidden %d is refused: %d B of LDS per %d-row chunk > 160 KB (the joint critic input is %d columns wide)", T.name, H,
                           lds_bytes_for(h, h.rc), h.rc, h.lds_kin_pad);
    if (whole_cu && h.state_dim > 0 && lds_bytes_for(h, h.rc) > 160 * 1024)
        return plan_refuse(message, "%s: %d B of LDS per row chunk > 160 KB (a first layer of %d input columns, %d of them the state's: state_dim)", T.name,
                           lds_bytes_for(h, h.rc), h.lds_kin_pad, h.state_dim);
    if (whole_cu && lds_bytes_for(h, h.rc) > 160 * 1024)
        return plan_refuse(message, "%s: %d B of LDS per row chunk > 160 KB (a first layer of %d input columns)", T.name, lds_bytes_for(h, h.rc), h.lds_kin_pad);
    if (lds_bytes_for(h, h.rc) > 160 * 1024) return plan_refuse(message, "network too wide for LDS (%d B at 16 rows)", lds_bytes_for(h, h.rc));
    if (T.two_wg && lds_bytes_for(h, h.rc) > 80 * 1024)
        return plan_refuse(message, "%s: %d B of LDS per row chunk > 80 KB (two workgroups per CU)", T.name, lds_bytes_for(h, h.rc));
    pl.lds_bytes = lds_bytes_for(h, h.rc);
    // Row chunks per gradient workgroup.  With `units` (learner, agent) pairs and n_chunks chunks each, s slabs per unit cost
    // ceil(units * s / slots) rounds of n_chunks / s chunk-times on the chip's resident-workgroup slots, and the reduce
    // pass streams s slabs: take the fewest slabs (but two) among the cheapest schedules.  512 learners x 4 chunks of 64
    // rows on 512 slots: two workgroups per learner walk 2 chunks each (2 slabs) instead of 4 workgroups writing 4 slabs.
    {
        const int n_chunks = (call_rows + h.rc - 1) / h.rc;
        // resident gradient workgroups: 256 CUs x (2 by registers — the kernels are built for FRL_GRAD_WGS = 2 — or 1 by LDS)
        const long long slots = 256LL * std::max(1, std::min(2, (160 * 1024) / std::max(1, pl.lds_bytes)));
        const long long units = (long long)h.P * h.n_agents;
        long long best_cost = -1;
        h.cps = 1;
        for (int cps = n_chunks; cps >= 1; --cps) {
            if (n_chunks % cps) continue;
            const int s = n_chunks / cps;
            // measured (P = 512, 4 chunks): 2 slabs 529 k updates/s, 1 slab 524 k, 4 slabs 495 k — with a single slab every
            // workgroup of the launch starts at once and they stay in step (gather bursts, barrier phases coincide)
            if (s < 2 && n_chunks >= 2) continue;
            const long long cost = ((units * s + slots - 1) / slots) * cps;
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; h.cps = cps; }
        }
        if (one_wg_per_net) h.cps = 1;
        if (knobs.cps >= 1 && n_chunks % knobs.cps == 0) h.cps = knobs.cps;      // developer knob
        h.S = n_chunks / h.cps;
    }
    if (!pl.has_nets) return FRL_OK;
    // the sizes of the buffers that hang on the nets
    const size_t P = h.P;
    h.Gmax = 1;
    for (int i = 0; i < h.n_nets; ++i) h.Gmax = std::max(h.Gmax, (h.net[i].size / 4 + 256 * kAdamVec - 1) / (256 * kAdamVec));
    pl.slab_count = slab_floats(h);
    pl.part_count = part_floats(h);
    pl.act_spill_count = c.algo == FRL_ALGO_CEM_GD3PG ? cem_spill_floats(h) : T.act_spill ? act_spill_floats(h) : 0;      // (CEM_GD3PG: a block per (learner, actor, slice))
    // the chained family's actor stage (chained_shape admits DDPG / TD3 / SAC only: each has one); allocated whatever FRL_ACTOR_PARK says
    pl.actor_park_count = pl.family == FAM_CHAINED ? actor_park_floats(h.P) : 0;
    pl.idx_count = P * h.n_agents * h.batch_max;
    if (h.noisy) {
        const LayerDesc& HL = h.net[0].L[h.net[0].n_layers - 1];
        pl.noisy_per_set = 2 * (HL.k_pad + HL.n_pad);
    }
    h.noise_sets = c.algo == FRL_ALGO_MASAC ? 2 * h.n_agents + 1 : std::max(2, h.n_agents);      // (MASAC: frl_desc.h, EngineDesc::noise_sets)
    pl.alpha_count = P * (c.algo == FRL_ALGO_MASAC ? (size_t)h.n_agents : 1) * 4;
    pl.steps_count = P * (kMaxNets + 1) + (c.algo == FRL_ALGO_MASAC ? P * (size_t)h.n_agents : 0);
    pl.noise_count = P * h.n_agents * h.noise_sets * (size_t)h.batch_max * h.act_max;
    int biggest = 0;
    for (int i = 0; i < h.n_nets; ++i) biggest = std::max(biggest, h.net[i].size);
    if (h.solo || h.solow) {
        pl.solo_stride = biggest;
        // (kernels_solow.hip: helper workgroups on the CUs a small population leaves idle take a share of the slab sum and of Adam —
        //  FRL_SOLOW_HELPERS=0 switches them off; every workgroup of a launch must be resident)
        pl.solow_wgs = h.solow ? h.solow : kSoloWG;      // (kernels_solow.hip: row tiles per unit)
        if (h.solow) {
            const int rw = pl.solow_row_wgs, U = (int)(P * (size_t)h.n_agents);
            const int per = std::min(64 / rw > 0 ? 64 / rw : 1, std::max(1, pl.n_cus / (rw * U)));      // (at most 64 workgroups per unit: the mailboxes are polled by one wave)
            pl.solow_wgs = knobs.solow_helpers ? rw * per : rw;
        }
    }
    if (h.wide || h.solow) pl.act_wk_slot = P * (size_t)biggest;      // select_action's Wk-layout copies of the nets (launch_act)
    int omax = 1;
    for (int j = 0; j < c.n_agents; ++j) omax = std::max(omax, c.obs_dim[j]);
    h.obsnorm_w = 1 + 3 * omax;
    return FRL_OK;
}

// cfg (+ ext) on a device with `limits` under `knobs` -> the plan, or FRL_ERR_INVALID and why.  Safe on any input: the argument check
// runs first (frl_create_ex runs it on its own as well, ahead of its device check).
inline int plan_engine(const frl_config& c, const frl_config_ext* ext, const PlanLimits& limits, const PlanKnobs& knobs, EnginePlan* plan, std::string* message) {
    if (const int rc = check_create_args(c, ext, message)) return rc;
    const int state_dim = ext ? ext->state_dim : 0;
    *plan = EnginePlan();
    EnginePlan& pl = *plan;
    pl.n_cus = knobs.assume_cus > 0 ? knobs.assume_cus : limits.n_cus;
    pl.lds_per_cu = limits.lds_per_cu;
    EngineDesc& h = pl.h;
    memset(&h, 0, sizeof h);
    const AlgoTraits& T = algo_traits(c.algo);
    h.algo = c.algo;
    h.P = c.n_learners;
    h.n_agents = c.n_agents;
    h.hidden = c.hidden > 0 ? c.hidden : 128;
    pl.ring_cap = c.capacity;
    pl.n_rings = c.algo == FRL_ALGO_CEM_GD3PG ? 2 : 1;
    h.capacity = c.algo == FRL_ALGO_CEM_GD3PG ? (c.capacity <= (1 << 30) ? 2 * c.capacity : c.capacity) : c.capacity;      // (plan_refusals refuses the larger ones)
    h.batch_max = c.batch_max > 0 ? c.batch_max : 256;
    if (c.algo == FRL_ALGO_REINFORCE) h.batch_max = c.capacity;      // a call's batch is everything stored since the last one
    h.seed = c.seed;
    h.n_discrete = T.discrete_head ? c.act_dim[0] : 0;               // (PPO's and the MAPPO family's discrete heads: plan_nets)
    h.reward_dim = T.vector_reward ? std::max(1, c.reward_dim) : 1;
    h.state_dim = state_dim;
    h.state_rows = state_dim > 0 ? ext->state_rows : (int)FRL_STATE_ROWS_POSITION;
    pl.has_nets = c.algo != FRL_ALGO_REPLAY_ONLY;
    if (const int rc = plan_refusals(c, state_dim, h, message)) return rc;
    build_record(h.rec, c);
    h.state_off = state_dim > 0 ? h.rec.extra_off + h.rec.extra - state_dim : 0;
    plan_nets(c, state_dim, pl);
    return plan_sizes(c, knobs, pl, message);
}

}  // namespace frl
