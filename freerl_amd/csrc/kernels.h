// Argument structs and prototypes of every kernel of the library.  Each kernels_*.hip is its own translation unit
// (compiled in parallel by freerl_amd/_native.py:build; no relocatable device code needed: a kernel's device code is
// complete in the unit that defines it); the host API (frl_api.hip) launches them through these declarations.
#pragma once
#include <hip/hip_runtime.h>

#include "frl_desc.h"

#ifndef FRL_GRAD_WGS
#define FRL_GRAD_WGS 2      // gradient-kernel workgroups per CU the register budget is sized for (frl_create picks rc to match)
#endif

namespace frl {

// ---- kernels_act.hip
enum ActMode : int {
    ACTM_RAW = 0,        // head output as is (Q values, V(s), Gaussian mean before squashing)
    ACTM_ARGMAX = 1,     // DQN greedy action (index as float)
    ACTM_TANH = 2,       // tanh(head): deterministic actors, SAC/PPO evaluate_action
    ACTM_SAC_SAMPLE = 3, // tanh(mean + std*eps)
    ACTM_PPO_SAMPLE = 4, // a = tanh(head) + std*eps ; logp per dimension
    ACTM_CAT_SAMPLE = 5  // Categorical(softmax(head)).sample() = argmax(p / q), q ~ Exp(1); logp of the draw
};

struct ActArgs {
    int net;             // net index
    int use_target;
    int mode;
    int n_rows;          // rows per learner
    int head;            // critic head (0/1) for ACTM_RAW on twin critics
    int in_dim;          // logical input width (obs dim, or obs+act for critics)
    int normalize;       // apply Batch_ObsNorm to the first obs_dim input columns (policy / value nets on raw obs)
    const float* in;     // [P][n_rows][in_dim] dense
    const float* eps;    // [P][n_rows][out_dim] standard normal draws, or nullptr
    float* out;          // [P][n_rows][out_dim]   (ARGMAX: out_dim = 1)
    float* out_logp;     // [P][n_rows][out_dim] (PPO sample) or nullptr
    // ---- exploration folded into the launch (frl_act_explore, the rollout collectors).  env_out == nullptr: none of it runs.
    int explore;         // ExploreKind
    int device_eps;      // 1: the sampling modes draw their own N(0,1) / Exp(1) variates (Philox) instead of reading `eps`
    float epsilon;       // EXPL_EPS_GREEDY: P(random action)                                   (DQN.py:307-310)
    float sigma;         // EXPL_GAUSS: std of the action noise in units of max_action           (TD3.py:412 gauss_sigma)
    float scale0;        // multiplier of the Gaussian noise / of the OU state when `scale` is nullptr (gauss_scale, OUNoise.scale)
    float max_action;
    float ou_theta, ou_sigma, ou_dt;   // EXPL_OU: x += theta*(0 - x) + sqrt(dt)*sigma*N(0,1)     (SAC.py:334-356)
    const float* scale;  // [P] per-learner multiplier (the reference decays it per episode, TD3.py:425-427, SAC.py:548-551) or nullptr
    float* ou_state;     // [P][n_rows][out_dim]
    const unsigned char* flags;   // [P][n_rows] bit 1: the row's episode ended on the previous step -> OU state reset first (SAC.py:546-547)
    float* env_out;      // [P][n_rows][out_dim] env-unit action = clip(a*max_action + noise, +-max_action); discrete: [P][n_rows] index
    unsigned long long rng_counter;
    const float* theta_alt;   // non-null: [P][NetDesc::size] Wk-layout copy of the net to read instead of theta / target (frag_to_wk_kernel)
};
enum ExploreKind : int { EXPL_NONE = 0, EXPL_EPS_GREEDY = 1, EXPL_GAUSS = 2, EXPL_OU = 3 };

// ---- kernels_per.hip
constexpr int kPerSetMax = 4096;      // rows of one per_set_kernel launch (its later-entry-wins scan stages them in LDS)
struct PerArgs {
    double* sum_tree;      // [P][2*cap-1]
    double* max_tree;      // [P][2*cap-1]
    int cap;               // leaves per learner
    int n;                 // entries in this launch
    const int* leaf;       // [P][n_pitch] buffer indices to write (per_set) / out: sampled indices (per_sample writes D.idx)
    int n_pitch;
    const float* prio;     // per_set: [P][n_pitch] priorities, or nullptr: use `fill` for every entry
    double fill;
    const int* size;       // [P] rows valid per learner
    // sampling
    const double* uniforms;   // [P][n] draws in [0,1) or nullptr (Philox)
    float* isw;               // [P][batch_max] importance weights out
    float* prio_out;          // [P][batch_max] float32 priorities of the sampled leaves
    double beta;
    unsigned long long rng_counter;
    const float* td;          // per_update: [P][batch_max] TD errors -> priority (|td| + eps)^alpha in float32
    float alpha, eps;
};

// ---- kernels_ppo.hip
struct PpoArgs {
    int horizon, minibatch, k_epochs, adv_norm;
    float gamma, lmbda, clip, ent_coef;
    float actor_lr, critic_lr, adam_eps, beta1, beta2, clip_norm;
    int optimizer;    // 0 torch Adam per net, 1 PPO.py's cautious AdamW (lr = actor_lr for both nets)
    // device scratch, per learner blocks of `horizon` floats
    float* td;        // [P][T] td_delta, then (after GAE) unused
    float* vs;        // [P][T] V(s)
    float* adv_raw;   // [P][T] GAE advantages before normalisation
    float* adv;       // [P][T] advantages used by the surrogate
    float* vtarget;   // [P][T]
    float* trace;     // [P][k_epochs * n_mb][2] per-minibatch (actor, critic) losses
    const int* perm;  // [P][k_epochs][T]
    const float* last_value;   // [P] (gae_mode 1)
    double gamma_d, lmbda_d;   // the float64 scan's discount and lambda (gae_mode 1)
};

// ---- kernels_replay.hip
struct GatherFields {
    int n_fields;
    int col0[8];
    int ncols[8];
    float* out[8];        // out[f][b][ncols[f]] dense
};

// Rollout commit: one launch writes the transitions of a vector step into the ring(s) from what is already on the device
// (the observations the policy saw, the actions it chose, their log-probs) plus the one block the host uploaded after
// env.step (next_obs, obs_next, reward, flags, ring rows), and advances the device copy of the current observations.
struct CommitArgs {
    float* obs_cur;               // [n][O] in: obs of the transition; out: obs_next (what the policy sees next)
    const float* store_act;       // [n][aout] action as stored by add() (policy output in (-1,1) / action index)
    const float* logp;            // [n][n_logp] or nullptr
    const int* row;               // [n] ring row of env i inside its learner's ring
    const float* next_obs;        // [n][O]
    const float* obs_next;        // [n][O]
    const float* reward;          // [n]
    const unsigned char* flags;   // [n] bit 0 terminated (the stored `done`), bit 1 episode ended, bit 2 adv_done (PPO)
    int n, E, O, aout, n_logp;
};

// ---- kernels_update.hip: reduce + clip + Adam.  which = 0: critic / Q-net, 1: actor.
struct AdamArgs {
    int which, ns, batch, soft, sac_alpha, G, p0;
    float lr, eps, beta1, beta2, wd, clip, tau, alpha_lr, target_entropy;
    int ragged;          // 1 (frl_reinforce_learn): learner p's batch is its own EngineDesc::ep_n[p] rows — its slabs are the workgroups that
                         // had rows, and a learner with none is skipped whole (slabs, step count, moments, statistics untouched)
    int agent1;          // > 0 (MASAC's actor steps, one agent after the other): the launch's units are LEARNERS and every one of them steps
                         // agent agent1 - 1; 0: units = (learner, agent) pairs.  sac_alpha = 2 with it: that agent's own alpha step
};
// (kAdamVec, float4 per thread per workgroup of reduce_kernel / adam_kernel: frl_desc.h)
constexpr int kFusedThreads = 1024, kFusedVec = 12;      // adam_fused_kernel: one workgroup per net, gradient in registers
constexpr int kFusedVecWide = 18;                        // adam_fused_wide_kernel: nets up to 73 k parameters (element-major slab sums)

// kernels_act.hip
__global__ void act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a);
__global__ void act_frag_kernel(const EngineDesc* __restrict__ Dp, ActArgs a);

// kernels_actor.hip
__global__ void ac_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);

// kernels_c51.hip
__global__ void c51_grad_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);

// kernels_critic.hip
__global__ void ac_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);

// kernels_sacd.hip: discrete SAC (SAC_file/SAC_add_discrete.py), row-chunk gradient kernels
__global__ void sacd_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);
__global__ void sacd_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);

// kernels_reinforce.hip: REINFORCE (REINFORCE_file/REINFORCE.py), the episode's return scan and the policy-gradient kernel
__global__ void reinforce_returns_kernel(const EngineDesc* __restrict__ Dp, double gamma);
__global__ void reinforce_grad_kernel(const EngineDesc* __restrict__ Dp, int p0, int p_count, int ns);

// kernels_envelope.hip: envelope multi-objective DQN (ENVELOPE_MORL_file/ENVELOPE_DQN.py), row-chunk gradient kernel over batch x weight_num rows
struct EnvelopeArgs {
    int batch, weight_num;            // B sampled ring rows x W preference vectors = B W rows
    int draw_w;                       // 1: envelope_weights_kernel draws the preferences (Philox); 0: EngineDesc::env_w as uploaded
    float gamma, beta;
    unsigned long long rng_counter;
    int p0, p_count;
};
__global__ void envelope_weights_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a);
__global__ void envelope_grad_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a, int ns);

// kernels_envelope_ddpg.hip: envelope multi-objective DDPG (ENVELOPE_MORL_file/ENVELOPE_DDPG.py), the critic and actor gradient kernels
// over the same batch x weight_num rows (EnvelopeArgs; envelope_weights_kernel expands the rows and draws the preferences)
__global__ void envelope_ddpg_critic_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a, int ns);
__global__ void envelope_ddpg_actor_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a, int ns);

// kernels_gail.hip: GAIL's discriminator (GAIL_file/GAIL.py): E expert ring rows + N staged policy rows per call
struct GailArgs {
    int n_expert, n_policy;           // E, N
    int gp;                           // 0: sigmoid + BCE; 1: logits, 0.5 x BCE-with-logits + gp_weight x gradient penalty on the expert rows
    int size;                         // gail_draw_kernel: rows valid in every ring
    float gp_weight;
    unsigned long long rng_counter;
    int p0, p_count;
};
__global__ void gail_draw_kernel(const EngineDesc* __restrict__ Dp, GailArgs a);
__global__ void gail_disc_kernel(const EngineDesc* __restrict__ Dp, GailArgs a, int ns);
__global__ void gail_stats_kernel(const EngineDesc* __restrict__ Dp, GailArgs a, int ns);
__global__ void gail_forward_kernel(const EngineDesc* __restrict__ Dp, int mode, int n_rows, const float* __restrict__ in, float* __restrict__ out);

// kernels_gail_ppo.hip: GAIL's policy side (GAIL_file/PPO2.py) on an ALGO_GAIL_PPO engine
struct GailPpoArgs {
    int horizon, minibatch, k_epochs;
    float gamma, c;            // c = float32(double(gamma) * double(lam)), as torch forms `gamma * lam * masks_2[t]`
    float clip, ent_weight, value_loss_coef;
    float p_lr, v_lr, clip_norm;
    float* vs;                 // [P][T] V(s_t) before the update
    float* logp_old;           // [P][T] log pi_old(a_t | s_t), summed over dimensions
    float* td;                 // [P][T] td_t
    float* adv_raw;            // [P][T] advantages before normalisation
    float* adv;                // [P][T] normalised
    float* returns;            // [P][T] adv_raw + V
    float* trace;              // [P][k_epochs * n_mb][2]
    const int* perm;           // [P][k_epochs][T]
    const float* last_value;   // [P] device
    const float* rewards;      // [P][T] device, or nullptr: the ring's reward column
};
__global__ void gail_ppo_prepare_kernel(const EngineDesc* __restrict__ Dp, GailPpoArgs a);
__global__ void gail_ppo_gae_kernel(const EngineDesc* __restrict__ Dp, GailPpoArgs a);
__global__ void gail_ppo_update_kernel(const EngineDesc* __restrict__ Dp, GailPpoArgs a);
__global__ void gail_ppo_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a);

// kernels_cem_gd3pg.hip: CEM_GD3PG (CEM_GD3PG_file/CEM_GD3PG.py) on an ALGO_CEM_GD3PG engine: net 0 actor_1, net 1 actor_2, net 2 the critic,
// net 3 actor_domain.  The batch is rows = 2 x half absolute ring rows in EngineDesc::idx: `half` of ring 0, then `half` of ring 1
struct CemArgs {
    int rows, half;               // B = 2 half rows of a call
    int size1;                    // cem_draw_kernel: both halves are drawn below this (rows valid in every learner's ring 1)
    int ring_cap;                 // rows of one ring: ring 1's row r is absolute row ring_cap + r
    float gamma, lambda;
    float tau, actor_lr, critic_lr;
    int stage;                    // cem_step_kernel: 0 the critic (units = learners), 1 both actors (units = (learner, actor))
    unsigned long long rng_counter;
    int p0, p_count;
};
__global__ void cem_draw_kernel(const EngineDesc* __restrict__ Dp, CemArgs a);
__global__ void cem_critic_kernel(const EngineDesc* __restrict__ Dp, CemArgs a, int ns);
__global__ void cem_actor_kernel(const EngineDesc* __restrict__ Dp, CemArgs a, int ns);
__global__ void cem_step_kernel(const EngineDesc* __restrict__ Dp, CemArgs a, int ns);
__global__ void cem_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a);

// kernels_mappo.hip: MAPPO / IPPO (MAPPO_file/MAPPO.py, IPPO.py): a unit = (learner, agent); nets 2i / 2i+1 = agent i's actor / critic
struct MappoArgs {
    int horizon, minibatch, k_epochs, adv_norm;
    int huber;            // critic loss: 0 F.mse_loss, 1 huber_loss(e, huber_delta).mean()
    float gamma, lmbda, clip, ent_coef;
    float actor_lr, critic_lr, adam_eps, beta1, beta2, clip_norm, huber_delta;
    float* td;            // [P * n][T] td_delta of agent i's critic, reward and done columns
    float* advd;          // [P * n][T] agent i's adv_done column, dense (gae_dense_kernel reads it)
    float* vs;            // [P * n][T] V_i(s)
    float* adv_seq;       // [P * n][T] the scan's output
    float* adv_raw;       // [P][T][n] advantages before normalisation
    float* adv;           // [P][T][n] advantages the surrogate uses
    float* vtarget;       // [P][T][n]
    float* trace;         // [P][n][k_epochs * n_mb][2] (actor, critic) loss of every step
    const int* perm;      // [P][n][k_epochs][T]
};
__global__ void mappo_values_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a);
__global__ void mappo_adv_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a);
__global__ void mappo_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a);
__global__ void mappo_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a);

// kernels_mappo_mask.hip: action-masked MAPPO (MAPPO_file/MAPPO_for_mask_action.py) on a FRL_ALGO_MAPPO engine with EngineDesc::mask_off set
__global__ void mappo_mask_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a);
__global__ void mappo_mask_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a, const float* __restrict__ mask);

// kernels_mappo_state.hip: MAPPO with a global-state critic (MAPPO_file/MAPPO_for_mask_action_state.py) on a FRL_ALGO_MAPPO engine with
// EngineDesc::state_dim > 0 (frl_create_ex); the second update kernel when EngineDesc::mask_off is set as well
__global__ void mappo_state_values_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a);
__global__ void mappo_state_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a);
__global__ void mappo_state_mask_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a);

// kernels_att.hip: ATT-MADDPG (MADDPG_file/MADDPG_simple_with_tricks.py with trick['ATT'], ATT.py): the attention critic's gradient kernels
// of an ALGO_MADDPG_ATT engine in the row-chunk launch shape, and the critic's forward for frl_act
__global__ void att_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);
__global__ void att_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);
__global__ void att_q_kernel(const EngineDesc* __restrict__ Dp, ActArgs a);

// kernels_masac.hip: MASAC (MAAC_file/MASAC.py): the gradient kernels of an ALGO_MASAC engine in the row-chunk launch shape — the critic
// launch over (learner, agent) units, the actor launch over learners for the ONE agent LearnArgs::agent — and the stacked
// [mean | log_std] head's forward for frl_act (FRL_ACT_TANHHEAD / FRL_ACT_SAC_SAMPLE)
__global__ void masac_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);
__global__ void masac_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);
__global__ void masac_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a);

// kernels_happo.hip: HAPPO (MAPPO_file/HAPPO.py): one launch per visiting position, after MAPPO's three advantage launches
struct HappoArgs {
    const int* order;     // [P][n] the agent visited at each position
    float* old;           // [P][T] sum_c log pi(a | o) of the visited agent's actor before its steps
    float* factor;        // [P][n][T] by visiting position: the product of the earlier visited agents' new-over-old policy ratios
    int k;                // this launch's visiting position
};
__global__ void happo_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a, HappoArgs x);

// kernels_dqn.hip
__global__ void dqn_grad_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns);

// kernels_noisy.hip
__global__ void noisy_materialise_kernel(const EngineDesc* __restrict__ Dp, int set0, int n_sets, int target_mask);
__global__ void noisy_draw_kernel(const EngineDesc* __restrict__ Dp, int set0, int n_sets, unsigned long long counter);

__global__ void per_add_kernel(PerArgs a, const int* __restrict__ bucket, int P);
__global__ void per_set_kernel(const EngineDesc* __restrict__ Dp, PerArgs a);
__global__ void per_sample_kernel(const EngineDesc* __restrict__ Dp, PerArgs a);

// kernels_ppo.hip
__global__ void ppo_values_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a);
__global__ void ppo_gae_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a);
__global__ void ppo_gae_sb3_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a);
__global__ void ppo_perm_kernel(int* __restrict__ perm, int T, int Tpad, unsigned long long counter, unsigned long long seed);
__global__ void gae_dense_kernel(const float* __restrict__ delta, const float* __restrict__ adv_done, int T, float c, float* __restrict__ adv);
__global__ void ppo_update_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a);

// kernels_replay.hip
__global__ void replay_scatter_kernel(float* __restrict__ ring, const float* __restrict__ staged, const long long* __restrict__ slots, int n, int width, int stride);
__global__ void replay_gather_kernel(const float* __restrict__ ring, const long long* __restrict__ idx, int B, int stride, GatherFields F);
__global__ void replay_read_kernel(const float* __restrict__ ring, long long row0, int n, int width, int stride, float* __restrict__ out);
__global__ void replay_commit_kernel(float* __restrict__ ring, RecordDesc rec, int capacity, CommitArgs c);
__global__ void replay_fill_kernel(float* __restrict__ ring, long long rows, RecordDesc rec, int n_discrete, unsigned long long seed);

// kernels_her.hip: hindsight relabelling of finished episodes inside the ring (frl_her_relabel; addressing: her_plan.h)
enum HerEp : int { HER_EP_LEARNER = 0, HER_EP_L = 1, HER_EP_CURSOR = 2, HER_EP_PICK0 = 3, HER_EP_ACT0 = 4, HER_EP_INTS = 5 };
struct HerArgs {
    const int* eps;               // [n_episodes][HER_EP_INTS]: learner, L, cursor before the call, first entry of `picks`, first row of `env_actions`
    const int* picks;             // [sum total] offset in [0, m_i) of every output row, or nullptr: drawn here (Philox, Floyd's k-subset)
    const float* env_actions;     // [sum L][A] the action column block of the relabelled rows, or nullptr: the source row's stored action
    const double* weights;        // [G]
    double tolerance;
    int capacity, S, G, A, sample_num, sample_range, mode;      // mode 0: reward = cost < tolerance ? 0 : -1; 1: reward = -cost
    unsigned long long counter, seed;                           // device draws: the relabel call's number, the engine's key
};
__global__ void her_relabel_kernel(float* __restrict__ ring, RecordDesc rec, HerArgs a);

// kernels_update.hip
__global__ void relayout_to_wk_kernel(const EngineDesc* __restrict__ Dp, float* scratch);      // scratch: [4][P][learner_stride]
__global__ void frag_to_wk_kernel(const EngineDesc* __restrict__ Dp, int net, int use_target, float* dst);   // dst: [P][NetDesc::size]
__global__ void draw_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int want_noise);
__global__ void obsnorm_kernel(const EngineDesc* __restrict__ Dp, int batch, int all_rows, int p0);
__global__ void reduce_kernel(const EngineDesc* __restrict__ Dp, AdamArgs a);
__global__ void adam_kernel(const EngineDesc* __restrict__ Dp, AdamArgs a);
__global__ void adam_fused_kernel(const EngineDesc* __restrict__ Dp, AdamArgs a);
__global__ void adam_fused_wide_kernel(const EngineDesc* __restrict__ Dp, AdamArgs a);
__global__ void soft_update_kernel(const EngineDesc* __restrict__ Dp, float tau, int p0);

// kernels_critic2.hip: the critic stage of DDPG / TD3 / SAC for one learner per workgroup (register-chained, Adam fused)
__global__ void ac_critic_v2_twin_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_v2_single_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_v2_twin_nv_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);      // (_nv: aligned next_obs / (reward, done) loads)
__global__ void ac_critic_v2_single_nv_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
// (round 2-5's four-wave form of the same stage, one wave per SIMD: FRL_CHAIN_WAVES=4, same-box A/B runs)
__global__ void ac_critic_v2w4_twin_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_v2w4_single_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);

// kernels_criticw.hip / kernels_actorw.hip: the same two stages on the K-sliced chained design (device/chain_wide.hpp) for wide
// first layers / heads and multi-agent critics; h<critic heads>a<actor head tiles>
__global__ void ac_critic_wide_h1a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_wide_h1a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_wide_h2a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_wide_h2a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_actor_wide_a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_actor_wide_a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);

// kernels_criticx.hip / kernels_actorx.hip: ... and at hidden 256 (device/chain_wide16.hpp)
__global__ void ac_critic_x_h1a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_x_h1a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_x_h2a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_critic_x_h2a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_actor_x_a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_actor_x_a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);

// kernels_actor2.hip: the actor stage of DDPG / TD3 likewise
__global__ void ac_actor_v2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);
__global__ void ac_actor_v2_recompute_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);      // (FRL_ACTOR_PARK=0)
__global__ void ac_actor_v2w4_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a);

// ---- kernels_solo.hip: a single learner's DDPG / TD3 / SAC update on kSoloWG workgroups (device/solo.hpp)
struct SoloArgs {
    float* slab;            // [P][kSoloWG][slab_stride] partial gradients of the net being trained, fragment-image order
    float* part;            // [P][kSoloWG][8] per-workgroup partial sums: 0 loss / Q sum, 1 log-pi sum, 2 squared gradient norm
    unsigned* bar;          // [P][kSoloWG] "my slab is written" flags: the epoch of the last launch that wrote it
    int* err;               // [1] set to 1 by a barrier that timed out (a workgroup of the learner never arrived)
    unsigned bar_base;      // epoch of this launch = bar_base + kSoloWG (the host advances bar_base by kSoloWG per launch)
    int slab_stride;
    // The NEXT call's batch rows, drawn by a spare workgroup of THIS launch on a CU the learner's sixteen leave idle (round 6: the
    // draw was 6.5 us at the head of every critic launch's critical path).  Two slots per learner of kSoloPre ints, alternating by
    // launch: [0..1] the Philox counter the rows were drawn for, [2] the ring size, [3] the batch, [8 ..) the rows.  A launch uses
    // pre_read only if all three match its own arguments — same draw_indices(), same bits — and draws for itself otherwise.
    const int* pre_read;    // [P][kSoloPre] or NULL
    int* pre_write;         // [P][kSoloPre] or NULL: the grid carries p_count extra workgroups behind the learners'
    unsigned long long pre_counter;   // the counter the next frl_learn call will take if nothing else draws in between
    int tiles;              // kernels_solow.hip: row tiles = slabs = flags per unit (16: batches of up to 256 rows; 64: MADDPG's 1024); slab / bar are [units][tiles]
    unsigned* bar2;         // kernels_solow.hip, fused policy step: [units][64] "critic stepped" flags of the unit's helper workgroups (or NULL)
    int row_wgs;            // kernels_solow.hip: workgroups per unit that own row tiles (tiles / row_wgs each; flags are polled for these)
    int update_wgs;         // kernels_solow.hip: workgroups per learner in the grid (16 with row tiles + helpers that only take a share of the update); `part` is [P][update_wgs][..]
};
constexpr int kSoloPre = 8 + 256;
// The rollout loop's step folded into these launches (frl_rollout; what dqn_fused_kernel does for DQN): `head` — Buffer.add of the
// vector step's transitions at the start of the critic launch (every workgroup of the learner writes the same ring rows: it
// samples from them next) — and `tail` — at the end of the step's LAST launch: the device copy of the current observations moves
// on to obs_next, select_action + the exploration rule run on it (kernels_act.hip's own act_frag_body: the same draws, bit for
// bit, as the separate act launch), the env actions land in host memory and a host-visible word is flagged.
struct SoloStepArgs {
    int head, tail, act;          // act: the tail also selects the next actions (0 on a rollout call's last step)
    CommitArgs c;                 // c.obs_cur / store_act / row / next_obs / obs_next / reward / flags, n = P * E
    ActArgs act_args;             // as launch_act would have built them for the separate launch (in = c.obs_cur)
    int* ticket;                  // [1] learners that have finished their tail (zero between launches)
    int* done_flag;               // host-visible word (or nullptr): set to done_value once every learner's env actions are out
    int done_value;
    unsigned* bar2;               // [P][kSoloWG] "my slice of the actor is stepped" flags (the tail reads the whole actor)
    const int* go_flag;           // pre-armed launch (DqnStepArgs::go_flag; on the pool's second stream): the critic launch draws its rows, waits
    int go_value;                 // until dev_cnt has reached dev_wait (every workgroup of the step in front has left), stages its first image, then
    int* dev_cnt;                 // spins on this host-visible word until it holds go_value (-1: the host gave the step up, nothing is touched).
    int dev_wait;                 // dev_cnt: device word (or nullptr) every workgroup of a folded step's launches adds one to on its way out
};
__global__ void solo_critic_twin_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s, SoloStepArgs st);
__global__ void solo_critic_single_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s, SoloStepArgs st);
__global__ void solo_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s, SoloStepArgs st);
// ... with eight workgroups per learner, two row tiles each (populations of 17 .. 32 learners)
__global__ void solo_critic_twin_w8_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s, SoloStepArgs st);
__global__ void solo_critic_single_w8_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s, SoloStepArgs st);
__global__ void solo_actor_w8_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s, SoloStepArgs st);
// kernels_solow.hip: the same decomposition for wide first layers / heads of up to 32 outputs (device/solo_wide.hpp), behind draw_kernel;
// h<critic heads>a<actor head tiles>
__global__ void solow_critic_h1a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_critic_h1a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_critic_h2a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_critic_h2a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_actor_a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_actor_a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
// ... MADDPG / MATD3: a unit = (learner, agent)
__global__ void solow_critic_ma_h1a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_critic_ma_h1a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_critic_ma_h2a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_critic_ma_h2a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_actor_ma_a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_actor_ma_a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
// ... a policy step (critic + actor stage) of single-agent engines with helper workgroups in one launch
__global__ void solow_step_h1a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_step_h1a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_step_h2a1_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
__global__ void solow_step_h2a2_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, SoloArgs s);
// kernels_dqn2.hip: draw + DQN / Double-DQN update + Adam + soft update of one learner in one launch
// The rollout loop's neighbours of learn() folded into the same launch (frl_rollout, DQN.py:294-339): add() of the vector
// step's transitions before the sample, select_action + epsilon-greedy on the post-update net for the next step after it.
struct DqnStepArgs {
    int commit, act;              // which of the two run (0 / 0: plain learn())
    int E, O;                     // envs per learner, obs_dim
    const float* obs_cur;         // [P*E][O] obs of the transition
    const float* store_act;       // [P*E] action index as stored by add()
    const int* row;               // [P*E] ring row of env i inside its learner's ring
    const float* next_obs;        // [P*E][O] observation the transition ended in
    const float* obs_next;        // [P*E][O] observation the policy sees next (the reset observation after an episode end)
    const float* reward;          // [P*E]
    const unsigned char* flags;   // [P*E] bit 0 terminated
    float* act_out;               // [P*E] explored action index (what the next add() stores)
    float* env_out;               // [P*E] the same, for the env
    float epsilon;
    unsigned long long act_counter;   // Philox counter of the act draw (act_kernel's stream 0x9000)
    int* done_flag;               // host-visible word (or nullptr): set to done_value once env_out is written, so that the
    int done_value;               // host can pick the actions up without waiting for the launch to retire
    // PRE-ARMED launch (frl_rollout, small populations): the launch is enqueued a vector step AHEAD on the pool's second stream, so it
    // starts while the previous step's launch is still running: it draws the batch's rows (launch arguments only), waits on the DEVICE
    // word dev_done for the previous launch's done_value (that launch's parameters are final), stages both nets, then spins on the
    // host-visible word go_flag until the host — env stepped, block filled — sets it to go_value: launch latency, the gap between two
    // launches of a stream, the draw and the weight staging all run under the previous launch and the host's turn.  -1 in go_flag: the
    // host gave the step up, the launch returns without having touched anything.
    const int* go_flag;
    int go_value;
    int* dev_done;                // device word (or nullptr): set to done_value together with done_flag
    int dev_wait;                 // pre-armed: the done_value of the launch in front
    int* err;                     // pinned word (or nullptr): set to 2 when a pre-armed launch gives up after 2 s of waiting (NOT when the host cancels it):
};                                // its update and the next actions were dropped — frl_rollout / frl_sync report FRL_ERR_STATE instead of stepping the envs on stale actions
__global__ void dqn_fused_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, DqnStepArgs s);

// kernels_ppo2.hip: the on-chip variant of ppo_update_kernel, <first-layer k-blocks, hidden activation>
__global__ void ppo_update_v2_k1_relu(const EngineDesc* __restrict__ Dp, PpoArgs a);
__global__ void ppo_update_v2_k2_relu(const EngineDesc* __restrict__ Dp, PpoArgs a);
__global__ void ppo_update_v2_k1_tanh(const EngineDesc* __restrict__ Dp, PpoArgs a);
__global__ void ppo_update_v2_k2_tanh(const EngineDesc* __restrict__ Dp, PpoArgs a);
constexpr int ppo2_lds_floats(int k0b) { return 8 * k0b * 256 + 64 * 256 + 8 * 256 + 2 * 8192 + 128 + 128 + 16 + 16 + 96; }

}  // namespace frl
