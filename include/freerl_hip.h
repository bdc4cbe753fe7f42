/* freerl_hip.h — C ABI of the MI355X-native replay-sample + batched-update engine.
 *
 * FreeRL (the reference) is pure Python and has NO plugin / FFI interface: its
 * boundary for this path is the duck-typed class surface `Buffer.add / Buffer.sample /
 * Agent.update_* / <ALGO>.select_action / <ALGO>.learn`.  This header is what a ctypes (or
 * cffi / pybind) binding on the reference side binds in order to keep that surface and run it
 * on hand-written HIP kernels; `freerl_amd/` is exactly such a binding and INTEGRATION.md shows
 * the stub.  Each entry point names the reference interface it replaces (paths relative to
 * the FreeRL tree).
 *
 * Conventions: opaque handle, `int` status (0 = FRL_OK), no exceptions or torch types across
 * the boundary, plain pointers + sizes, caller-allocated output buffers.  One engine = one HIP
 * stream; an engine is thread-compatible (one thread at a time).  "host" pointers are ordinary
 * process memory, "device" pointers are HIP device memory on the engine's GPU.
 *
 * An engine holds P independent learners ("population": seeds / env-instance sets on this
 * GPU); P = 1 is the reference-compatible single learner.  Every call below
 * that takes [P][...] arrays processes all learners in ONE kernel launch.
 */
#ifndef FREERL_HIP_H
#define FREERL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRL_MAX_AGENTS 8
#define FRL_STAT_COUNT 8

enum frl_status { FRL_OK = 0, FRL_ERR_INVALID = 1, FRL_ERR_HIP = 2, FRL_ERR_NO_DEVICE = 3, FRL_ERR_STATE = 4 };

enum frl_algo {
    FRL_ALGO_REPLAY_ONLY = -1, /* stand-alone Buffer.py replacement, no networks */
    FRL_ALGO_DQN = 0,          /* DQN_file/DQN.py:62-138 */
    FRL_ALGO_DDPG = 1,         /* DDPG_file/DDPG_simple.py:100-179, DDPG.py */
    FRL_ALGO_TD3 = 2,          /* TD3_file/TD3.py:150-256 */
    FRL_ALGO_SAC = 3,          /* SAC_file/SAC.py:171-282 */
    FRL_ALGO_MADDPG = 4,       /* MADDPG_file/MADDPG_simple.py:107-210 */
    FRL_ALGO_PPO = 5,          /* PPO_file/PPO_with_tricks.py:211-374, PPO.py */
    FRL_ALGO_SAC_DISCRETE = 6, /* SAC_file/SAC_add_discrete.py:137-348 (is_continue=False): softmax actor, twin critics with one
                                  value per action; one agent, actions stored as one float index, act_dim[0] = number of actions */
    FRL_ALGO_REINFORCE = 7,    /* REINFORCE_file/REINFORCE.py:32-127: one net (index 0) obs -> hidden (ReLU) -> n_actions, softmax in the
                                  kernels; one agent, actions stored as one float index, act_dim[0] = number of actions (<= 64), hidden
                                  <= 256.  capacity = the most steps stored between two frl_reinforce_learn calls, and batch_max follows
                                  it.  The engine has NO target net: FRL_PARAM_TARGET addresses a block that frl_params_set / _get store and
                                  return but that no kernel of this algorithm reads or writes (frl_act with use_target = 1 runs on it) */
    FRL_ALGO_ENVELOPE_DQN = 8, /* ENVELOPE_MORL_file/ENVELOPE_DQN.py:36-266: one Q-net (index 0) [obs | preference] -> hidden (ReLU) -> hidden
                                  (ReLU) -> n_actions x reward_dim (column a * reward_dim + k = objective k of action a) with a target net;
                                  one agent, actions stored as one float index, act_dim[0] = number of actions, frl_config.reward_dim
                                  objectives: a record carries reward_dim reward columns (done_off = rew_off + reward_dim).  n_actions x
                                  reward_dim <= 64, hidden <= 256, and batch_max counts ROWS = batch x weight_num of frl_envelope_learn */
    FRL_ALGO_ENVELOPE_DDPG = 9,/* ENVELOPE_MORL_file/ENVELOPE_DDPG.py:40-320: net 0 the actor [obs | preference] -> hidden (ReLU) -> hidden
                                  (ReLU) -> act_dim[0] (tanh), net 1 the critic [obs | action | preference] -> hidden (ReLU) -> hidden
                                  (ReLU) -> reward_dim (linear), each with a target net; one agent, continuous actions stored as
                                  act_dim[0] floats, frl_config.reward_dim objectives and reward columns as on envelope-DQN engines.
                                  hidden <= 256, and batch_max counts ROWS = batch x weight_num of frl_envelope_ddpg_learn */
    FRL_ALGO_GAIL = 10,        /* GAIL_file/GAIL.py:17-120, the discriminator: one net (index 0) [obs | act] -> hidden -> hidden -> 1 with
                                  frl_config.hidden_act = FRL_ACT_LEAKY_RELU (slope 0.01, the reference's) or FRL_ACT_RELU, a linear head and
                                  NO target net (FRL_PARAM_TARGET as on REINFORCE engines).  One agent, continuous actions.  The ring holds
                                  the EXPERT rows in the standard record layout, of which only the obs and act columns are read: capacity
                                  = the number of expert rows, batch_max = the most rows of EITHER kind (expert, policy) one
                                  frl_gail_learn call may use.  hidden <= 256 */
    FRL_ALGO_MAPPO = 11,       /* MAPPO_file/MAPPO.py:123-482: n_agents <= FRL_MAX_AGENTS agents, net 2i the actor of agent i on its own observation
                                  obs_dim[i] -> hidden (ReLU) -> hidden (ReLU) -> act_dim[i] (tanh mean + a log_std block, or the logits of
                                  `discrete`, as on PPO engines), net 2i+1 its critic on the CONCATENATION of every agent's observation
                                  -> hidden -> hidden -> 1.  No target nets (FRL_PARAM_TARGET as on REINFORCE engines).  Records use the
                                  multi-agent layout (per-agent reward and done columns); extra_cols = sum_i (log-prob columns of agent i:
                                  act_dim[i], or 1 when discrete) + n_agents: the log-prob blocks in agent order, then one adv_done
                                  column per agent.  capacity = horizon.  hidden <= 256, ReLU only, <= 64 discrete actions */
    FRL_ALGO_IPPO = 12,        /* MAPPO_file/IPPO.py:57-347: the same, but the critic of agent i takes agent i's OWN observation and every
                                  agent is an independent PPO learner */
    FRL_ALGO_HAPPO = 13,       /* MAPPO_file/HAPPO.py:128-458: a FRL_ALGO_MAPPO engine in every respect at create (nets, the critic on the
                                  concatenated observation, record layout, limits), for heterogeneous agents updated one after another
                                  in a random order: updated by frl_happo_learn, not by frl_mappo_learn */
    FRL_ALGO_MADDPG_ATT = 14,  /* MADDPG_file/MADDPG_simple_with_tricks.py with trick['ATT'] (ATT.py:81-103,181-229): a FRL_ALGO_MADDPG engine
                                  (records, net 2i the actor of agent i, frl_learn with the same arguments) whose net 2i+1 is agent i's
                                  ATTENTION critic with a target copy: encoder_input_fc on [all obs | a_i], decoder_input_fc on the other
                                  agents' actions, fc_encoder_input, 4 fc_encoder_heads, fc_decoder_input, a softmax over the heads'
                                  scores against the decoder, fc1, fc2.  2 <= n_agents <= FRL_MAX_AGENTS, continuous actions, no twin
                                  critic.  frl_act with FRL_ACT_RAW on net 2i+1 takes rows [all obs | all actions] and returns Q.
                                  frl_params_get / _set order of net 2i+1: fc_encoder_input, the 4 heads' weights stacked [4 hidden][hidden]
                                  then their biases [4 hidden], fc_decoder_input, encoder_input_fc, decoder_input_fc, fc1, fc2 */
    FRL_ALGO_MASAC = 15,       /* MAAC_file/MASAC.py:32-302 (entropy_way_c = entropy_way_a = action_way = '1', adaptive alpha): MADDPG's
                                  records and net numbering, updated by frl_learn.  Net 2i: agent i's tanh-Gaussian actor obs_dim[i] ->
                                  hidden -> hidden -> [mean_layer | log_std_layer] (ONE head of 2 act_dim[i] outputs, log_std clamped to
                                  [-20, 2] per row), with a target copy that the TD target samples from; net 2i+1: its twin critic on
                                  [all obs | all actions] (l1, l2, l3 and l1_2, l2_2, l3_2 in one net, one optimiser).  One alpha per
                                  (learner, agent): frl_alpha_get_agent / frl_alpha_set_agent.  Per frl_learn call, for agent 0, 1, ..
                                  in order: critic step (every target actor sampled, the agent's own log-prob and alpha in the target),
                                  actor step (fresh actions of ALL online actors — agents j < i as just stepped — through the agent's
                                  own twin critic, min(Q1, Q2), entropy from a second draw of its own actor), alpha step (target entropy
                                  -act_dim[i]; frl_learn_args.target_entropy is unused); then every target is soft-updated.
                                  frl_params_get / _set order: actor l1, l2, mean_layer (weight, bias), log_std_layer (weight, bias);
                                  critic l1, l2, l3, l1_2, l2_2, l3_2.  frl_act on net 2i: FRL_ACT_SAC_SAMPLE = tanh(mean + std eps),
                                  FRL_ACT_TANHHEAD = tanh(mean) (act_dim[i] columns), FRL_ACT_RAW = [mean | log_std]; on net 2i+1:
                                  FRL_ACT_RAW on rows [all obs | all actions] = Q of `head` 0 / 1, online or target.
                                  Refused at create: discrete, twin_critic = 0, hidden_act != FRL_ACT_RELU, a row chunk that does not
                                  fit a CU's LDS.  Refused at the call (FRL_ERR_STATE): frl_obsnorm_enable, use_policy_noise,
                                  frl_rollout, frl_act_explore.  frl_version() 111 */
    FRL_ALGO_GAIL_PPO = 16,    /* GAIL_file/PPO2.py:20-307, the policy side of GAIL (and PPO2.py's own loop): net 0 the actor obs_dim ->
                                  hidden -> hidden -> act_dim with tanh on the mean and a state-independent log_std [act_dim] (zeros at
                                  create) clamped to the ENGINE's range (frl_log_std_range_set; [-10, 2] at create, PPO2's shipped
                                  config), or, with discrete, the logits of Categorical(logits=); net 1 the critic obs_dim -> hidden ->
                                  hidden -> 1.  hidden_act FRL_ACT_LEAKY_RELU or FRL_ACT_RELU (FRL_ACT_TANH is refused), hidden <= 256,
                                  the standard record with extra_cols = 0: `done` holds 1 - mask, the next_obs block is never read.
                                  Updated by frl_gail_ppo_learn only.  frl_act: FRL_ACT_RAW (net 1: value; net 0: the head),
                                  FRL_ACT_TANHHEAD (pi(return_mean=True)), FRL_ACT_PPO_SAMPLE (mean + std eps under the engine's
                                  range, eps given or drawn), FRL_ACT_CAT_SAMPLE / FRL_ACT_ARGMAX (discrete).  frl_version() 113 */
    FRL_ALGO_CEM_GD3PG = 18    /* (17 is unassigned: frl_create refuses it as an unknown algo, which callers and the suite have relied on since
                                  frl_version 113.)  CEM_GD3PG_file/CEM_GD3PG.py:30-231, guided dual-actor DDPG: net 0 actor_1, net 1 actor_2 and net 3
                                  actor_domain obs_dim -> hidden (tanh) -> hidden (tanh) -> act_dim (tanh), net 2 the critic [obs | act] ->
                                  hidden (LeakyReLU 0.01) -> hidden (LeakyReLU 0.01) -> 1.  Nets 0-2 have a target net and Adam state;
                                  net 3 is frozen (no kernel writes it; its target and Adam blocks are never touched).  hidden_act must
                                  be FRL_ACT_TANH (the actors'; the critic is always LeakyReLU); discrete, twin_critic and n_agents != 1
                                  are refused.  TWO rings of `capacity` rows per learner, ring 0 `buffer` and ring 1 `buffer_domain`
                                  (frl_ring_add / frl_ring_cursor_get; the frl_buffer_* calls serve ring 0, and frl_buffer_read's rows
                                  [r capacity, (r + 1) capacity) are ring r), zero-filled at create.  Updated by frl_cem_gd3pg_learn
                                  only.  frl_act: FRL_ACT_TANHHEAD on nets 0, 1 and 3 (use_target on 0 and 1), FRL_ACT_RAW on net 2.
                                  frl_version() 114 */
};

enum frl_activation { FRL_ACT_NONE = 0, FRL_ACT_RELU = 1, FRL_ACT_TANH = 2,
                      FRL_ACT_LEAKY_RELU = 3 /* slope 0.01; FRL_ALGO_GAIL and FRL_ALGO_GAIL_PPO engines only (frl_create refuses it elsewhere) */ };

/* which copy of a net's parameters frl_params_get/set addresses.  FRL_PARAM_GRAD is a debugging view of the reduced
 * gradient block: PPO engines, noisy DQN engines and nets wider than the fused Adam kernel materialise it; the other
 * off-policy updates keep the reduced gradient in registers and leave this block untouched. */
enum frl_param_kind { FRL_PARAM_ONLINE = 0, FRL_PARAM_TARGET = 1, FRL_PARAM_ADAM_M = 2, FRL_PARAM_ADAM_V = 3, FRL_PARAM_GRAD = 4 };

/* frl_act modes */
enum frl_act_mode {
    FRL_ACT_RAW = 0,        /* head output: Q values (DQN.py:83), V(s) (PPO_with_tricks.py:304-305), Gaussian mean */
    FRL_ACT_ARGMAX = 1,     /* DQN.select_action, DQN.py:70-84 */
    FRL_ACT_TANHHEAD = 2,   /* TD3/DDPG/MADDPG select_action (TD3.py:163-170), SAC/PPO evaluate_action */
    FRL_ACT_SAC_SAMPLE = 3, /* SAC.select_action, SAC.py:192-198: tanh(mean + std*eps) */
    FRL_ACT_PPO_SAMPLE = 4, /* PPO.select_action, PPO_with_tricks.py:234-255: a = mean + std*eps, per-dim log-prob */
    FRL_ACT_CAT_SAMPLE = 5  /* discrete PPO (:249-251): Categorical(softmax).sample() = argmax(p/q), q ~ Exp(1) in eps
                               [P][n_rows][n_actions]; out / logp are [P][n_rows] (index as float, log-prob of the draw) */
};

/* OR into `mode`: skip Batch_ObsNorm for this call — the reference's evaluate_action does not normalise
 * although select_action does (SAC.py:200-204 vs :194-195; DDPG.py:173-181 vs :165-166) */
#define FRL_ACT_NO_OBSNORM 0x100

/* per-(learner, agent) statistics written by frl_learn; index into stats[.][FRL_STAT_COUNT] */
enum frl_stat {
    FRL_STAT_CRITIC_LOSS = 0, FRL_STAT_ACTOR_LOSS = 1, FRL_STAT_ALPHA_LOSS = 2, FRL_STAT_ALPHA = 3,
    FRL_STAT_CRITIC_GNORM = 4, FRL_STAT_ACTOR_GNORM = 5, FRL_STAT_ENTROPY = 6
};

typedef struct frl_engine frl_engine;

/* Constructor arguments; mirrors `<ALGO>(dim_info, is_continue, lrs, buffer_size, device, ...)`
 * (DQN.py:63-68, TD3.py:151-161, SAC.py:172-190, MADDPG_simple.py:108-120, PPO_with_tricks.py:212-232). */
typedef struct frl_config {
    int algo;                     /* enum frl_algo */
    int n_learners;               /* P >= 1 */
    int n_agents;                 /* 1, or the MADDPG agent count (<= FRL_MAX_AGENTS) */
    int obs_dim[FRL_MAX_AGENTS];
    int act_dim[FRL_MAX_AGENTS];  /* continuous: action width; discrete (DQN): number of actions */
    int discrete;                 /* 1: actions are stored as ONE float index (Buffer.py:3-9 act_dim vs action_dim) */
    int hidden;                   /* 128 = the reference's hard-coded width (DQN.py:38, TD3.py:53 ...) */
    int hidden_act;               /* FRL_ACT_RELU, or FRL_ACT_TANH for PPO trick['tanh']; FRL_ALGO_GAIL: FRL_ACT_LEAKY_RELU or FRL_ACT_RELU */
    int twin_critic;              /* Critic_TD3 / SAC Critic: l1..l6 in one module */
    int capacity;                 /* replay rows per learner (PPO: horizon) */
    int batch_max;                /* largest batch / minibatch a learn call will use */
    int extra_cols;               /* extra record columns (PPO: act_dim log-probs + 1 adv_done) */
    int actor_dist;               /* PPO, discrete: 0 Categorical(probs=softmax(l3)) (PPO_with_tricks.py:107-118,333-336), 2
                                     Categorical(logits=l3) (PPO_file/PPO.py:78-90,176,257: no clamp at float eps).
                                     PPO, continuous: 0 Gaussian `Actor` (PPO_with_tricks.py:79-108), 1 `Actor_Beta` (:120-151):
                                     the actor's head is [alpha_layer ; beta_layer] = 2*act_dim outputs, no log_std */
    int dueling;                  /* DQN trick['Dueling'] (DQN_with_tricks.py:60-79): the head is [V ; A] = 1 + n_actions outputs and
                                     Q = V + A - mean(A) */
    int noisy;                    /* DQN trick['Noisy'] (Noisy_net.py:17-76): the head (l2, or Dueling's V and A) is NoisyLinear: parameters
                                     mu + sigma, fresh factorised noise at every forward */
    int c51_atoms;                /* DQN trick['Categorical'] (DQN_with_tricks.py:82-158): atoms of the value distribution (51), 0 = off */
    float c51_vmin, c51_vmax;     /* its support [v_min, v_max] (-100, 100) */
    int device_id;
    uint64_t seed;                /* device Philox key (fast path only) */
    int reward_dim;               /* FRL_ALGO_ENVELOPE_DQN / _DDPG: objectives (reward columns per record, preference columns of the Q-net's input);
                                     0 means 1, and every other algorithm ignores it */
} frl_config;

/* What frl_config cannot grow to hold (its last field is pinned): the extension block of frl_create_ex.
 * state_dim > 0 (FRL_ALGO_MAPPO only): MAPPO_file/MAPPO_for_mask_action_state.py.  Every critic's first layer is sum_i obs_dim[i] +
 * state_dim columns wide and reads [obs_0 | .. | obs_{n-1} | state]; the state block is the LAST state_dim columns of a record's extra
 * block (frl_state_info), so extra_cols = the engine's columns without a state (log-probs, adv_done, optionally the mask blocks) +
 * state_dim.  On a discrete engine both widths are accepted, and the width alone does not say which was meant (no masks and a
 * state of S + sum act_dim columns, or masks and a state of S): the caller declares the mask blocks by calling frl_action_mask_set,
 * which refuses unless they fit in front of the state block.  state_rows says which ring row a critic STEP takes the state block of its minibatch row r from (frl_state_rows); the
 * value pass always reads V(s) = critic(obs(t), state(t)) and V(s') = critic(next_obs(t), state(t)): the same row, as the reference
 * does (:322-323). */
struct frl_config_ext {
    int size;                     /* sizeof(frl_config_ext): for later growth */
    int state_dim;                /* 0: no state (frl_create's engine exactly) */
    int state_rows;               /* enum frl_state_rows */
};
typedef struct frl_config_ext frl_config_ext;
enum frl_state_rows {
    FRL_STATE_ROWS_POSITION = 0,  /* the reference's (:371-373): `state` is not indexed, so row r of the one minibatch is
                                     [obs[perm[r]] | state[r]], regressed on v_target[perm[r]].  frl_mappo_learn then refuses
                                     minibatch != horizon, where the reference raises */
    FRL_STATE_ROWS_SAMPLE = 1     /* [obs[perm[r]] | state[perm[r]]]: the state of the sampled row; any minibatch */
};

/* Column layout of one replay record (all agents of one transition, fp32):
 * [obs_0..|act_0..|rew_0..|done_0..|next_obs_0..|extra] — see DESIGN.md "Data layout".  The reward block is one column per agent,
 * except on FRL_ALGO_ENVELOPE_DQN / _DDPG engines, where it is the reward VECTOR: done_off - rew_off = reward_dim columns. */
typedef struct frl_record_layout {
    int n_agents, width, stride;
    int obs_off[FRL_MAX_AGENTS], obs_dim[FRL_MAX_AGENTS];
    int act_off[FRL_MAX_AGENTS], act_dim[FRL_MAX_AGENTS];
    int rew_off, done_off;
    int next_obs_off[FRL_MAX_AGENTS];
    int extra_off, extra;
} frl_record_layout;

/* Arguments of one learn() call: `<ALGO>.learn(batch_size, gamma, tau, ...)`
 * (DQN.py:104, DDPG_simple.py:137, TD3.py:189, SAC.py:222, MADDPG_simple.py:165). */
typedef struct frl_learn_args {
    int batch;                 /* min(len(buffer), batch_size) is the caller's job (DQN.py:95-96) */
    int do_actor;              /* TD3 / MATD3: total_it % policy_freq == 0 (TD3.py:224, MATD3_simple.py:236,245: actor step
                                  AND target update); else 1 */
    int use_policy_noise;      /* TD3 / MATD3 realize['policy_noise'] (FRL_ALGO_MADDPG + twin_critic + these two = MATD3_simple.py) */
    float gamma, tau;
    float actor_lr, critic_lr; /* DQN: critic_lr = Qnet_lr */
    float alpha_lr;            /* SAC Alpha, 1e-4 (SAC.py:155) */
    float adam_eps;            /* 1e-8; 1e-5 with PPO trick['adam_eps'] */
    float critic_weight_decay; /* DDPG.py:131-134 supplement; 0 otherwise */
    float clip_norm;           /* clip_grad_norm_ max_norm 0.5 (TD3.py:140); <= 0: none (DQN.py:56-59) */
    float policy_noise, noise_clip, max_action, policy_noise_scale;   /* TD3.py:196-198 */
    float target_entropy;      /* SAC: -act_dim (SAC.py:160) */
    int double_dqn;            /* DQN trick['Double'] (DQN_with_tricks.py:263-265) */
    int per;                   /* DQN trick['PER'] (:276-279): rows and importance weights of the last frl_per_sample; the TD errors
                                  stay on the device for frl_per_update.  1 = the reference's arithmetic: its [B] weights times
                                  [B,1] squared errors broadcast to [B,B], so loss = mean(w) * mean(td^2); 2 = mean(w_i * td_i^2) */
    const float* noisy_eps;    /* noisy engines: host [P][3][S] factorised noise of the three forwards of learn() in the reference's
                                  order (online on s' when double_dqn, target on s', online on s); S = frl_noisy_eps_size(): per
                                  NoisyLinear eps_in[hidden] then eps_out[rows] = f(randn) (Noisy_net.py:66-76), V before A.  NULL:
                                  drawn on the device */
    const int64_t* idx;        /* host [P][n_agents][batch] rows drawn by the caller (np.random.choice,
                                  DQN.py:97) for bit-identical sampling; NULL: drawn on the device */
    const float* noise;        /* host [P][n_agents][S][batch][act_max], S = max(2, n_agents): N(0,1) draws the reference
                                  takes from torch's generator (TD3.py:197 slot 0; SAC.py:227 slot 0, :244 slot 1;
                                  MATD3_simple.py:200: slot j = randn_like(action[agent j]) inside agent i's sample());
                                  FRL_ALGO_MASAC: S = 2 n_agents + 1, per updating agent i in the reference's order: slot j =
                                  actor_target_j's rsample in sample() (MASAC.py:214), slot n + j = actor_j's in the actor loss (:254),
                                  slot 2n = the second draw of actor_i for the entropy (:261);
                                  NULL: drawn on the device */
    float* stats_out;          /* host [P][n_agents][FRL_STAT_COUNT] or NULL (NULL: call is asynchronous) */
    int loss_kind;             /* TD loss of the Q / critic update: FRL_LOSS_MSE = F.mse_loss, what every hot-path learn() of the
                                  reference uses (DQN.py:116, TD3.py:212, SAC.py:237); FRL_LOSS_HUBER = the reference's
                                  huber_loss(e, d).mean() (MAPPO_file/MAPPO.py:273-276): e^2/2 if |e| <= d else d(|e| - d/2) */
    float huber_delta;         /* d (MAPPO_attention.py:518 defaults to 10) */
} frl_learn_args;
enum frl_loss_kind { FRL_LOSS_MSE = 0, FRL_LOSS_HUBER = 1 };

/* ---------------------------------------------------------------- library / engine lifetime */
const char* frl_last_error(void);          /* message of the last failing call on this thread */
int frl_version(void);
int frl_device_count(int* n_out);
int frl_create(const frl_config* cfg, frl_engine** out);
/* frl_create with an extension block; ext == NULL or ext->state_dim == 0 builds frl_create's engine exactly (frl_create(cfg, out) is
 * frl_create_ex(cfg, NULL, out)).  FRL_ERR_INVALID: ext->size != sizeof(frl_config_ext), state_dim < 0, a state_rows outside
 * frl_state_rows, state_dim > 0 on any algorithm but FRL_ALGO_MAPPO, an extra_cols that cannot hold the state block behind the
 * log-prob and adv_done columns, or a first layer of sum obs_dim + state_dim columns whose row chunk does not fit the 160 KB of LDS. */
int frl_create_ex(const frl_config* cfg, const frl_config_ext* ext, frl_engine** out);
/* the engine's state width and the record column of its state block (extra_off + extra - state_dim); 0 and 0 on engines without one */
int frl_state_info(const frl_engine* e, int* state_dim_out, int* state_col_out);
int frl_destroy(frl_engine* e);
int frl_sync(frl_engine* e);               /* wait for the engine's stream */
int frl_lds_bytes(const frl_engine* e, int* bytes_out, int* row_chunk_out);
/* Which kernel family frl_learn() launches for this engine at `batch` rows: chained = 1 when the critic and actor stages run
 * as one workgroup per learner with the weights in LDS images (kernels_critic2.hip / kernels_actor2.hip), 0 for the row-chunk
 * kernels + reduce / Adam launches; the dynamic LDS bytes and the batch rows of one workgroup of that family.  16 (or 32) rows with
 * chained = 1: the sixteen-workgroups-per-learner families of small populations (kernels_solo.hip; kernels_solow.hip for wide first
 * layers and MADDPG: 160512 bytes of LDS). */
int frl_learn_path(const frl_engine* e, int batch, int* chained_out, int* lds_bytes_out, int* rows_per_workgroup_out);
/* 1: the actor stage this engine launches reads pass A's h2 back from its park buffer (the eight-wave chained kernel, unless the engine
 * was created under FRL_ACTOR_PARK=0); 0: every other actor kernel, the recompute form of that one included.  Read off the kernel
 * that frl_create resolved, not off the knob. */
int frl_actor_park(const frl_engine* e, int* parked_out);

/* ---------------------------------------------------------------- replay ring (Buffer.py)
 * Replaces class Buffer (TD3_file/Buffer.py:11-61 = DQN_file/Buffer.py:12-62) and
 * Buffer_for_PPO (PPO_file/Buffer.py:266-323). */
int frl_record_layout_get(const frl_engine* e, frl_record_layout* out);
/* Buffer.add (Buffer.py:28-38): one record (host, `width` floats) appended at the learner's cursor;
 * staged in pinned memory and pushed by the next flush / sample / learn. */
int frl_buffer_add(frl_engine* e, int learner, const float* record);
/* vectorised add: record i goes to learner learners[i] (NULL: all to learner 0 in order) */
int frl_buffer_add_batch(frl_engine* e, int n, const int* learners, const float* records);
int frl_buffer_flush(frl_engine* e);
/* Buffer._index / Buffer._size / __len__ / clear (Buffer.py:23-24,60-61; PPO Buffer.py:303-306) */
int frl_buffer_cursor_get(const frl_engine* e, int learner, int* index_out, int* size_out);
int frl_buffer_cursor_set(frl_engine* e, int learner, int index, int size);
/* Buffer.sample(indices) (Buffer.py:40-57): gather rows `idx` (host int64[B]) of one learner into
 * n_fields dense DEVICE tensors out[f][B][ncols[f]] = record[:, col0[f] : col0[f]+ncols[f]] — one launch. */
int frl_buffer_sample(frl_engine* e, int learner, const int64_t* idx, int batch, int n_fields, const int* col0,
                      const int* ncols, float* const* out_device);
/* read `n` whole records starting at ring row `row0` into host memory [n][width] (Buffer_for_PPO.all, views) */
int frl_buffer_read(frl_engine* e, int learner, int row0, int n, float* out_host);
/* synthetic fill of the first `rows` rows of every learner's ring (bench only) */
int frl_buffer_fill_synthetic(frl_engine* e, int rows, uint64_t seed);

/* ---------------------------------------------------------------- hindsight experience replay (DDPG_file/DDPG_simple_try_HER.py)
 * The script's loop at an episode's end (:421-428) for the listed learners in ONE launch.  A stored observation is
 * [state (state_dim) | goal (goal_dim)], the achieved goal of a transition is next_state[0:goal_dim].  Learner learners[e]'s episode
 * is the lengths[e] rows behind its ring cursor, in time order.  For i = 0 .. L-1 the candidates are transitions i .. i + m_i - 1
 * with m_i = min(sample_range, L - i); all of them in order when m_i < sample_num, else sample_num distinct ones
 * (random.sample; m_i == sample_num is a shuffle).  For every pick j one row is appended at the cursor:
 *   obs = [state_i | g], action = env_actions row i (NULL: the stored action), reward = calcu_reward(g, state_i), next_obs =
 *   [next_state_i | g], done = 0, g = next_state_j[0:goal_dim];
 * calcu_reward (:247-265): cost = sum_c weights[c] (g_c - s_c)^2 in float64, left to right, from the stored float32 values without
 * fused multiply-adds; FRL_HER_SPARSE: cost < tolerance ? 0 : -1; FRL_HER_SHAPING: -cost.  Afterwards the cursor of each listed
 * learner stands where rows_out[e] = sum_i min(sample_num, sample_range, L - i) calls of frl_buffer_add would have left it.
 * Staged adds are flushed first.  Asynchronous (the next synchronising call waits for it).
 * Refused before any launch, ring and cursors untouched — FRL_ERR_INVALID: n_episodes < 1 or > n_learners, NULL learners / lengths,
 * a learner out of range or listed twice, sample_num outside [1, 8], sample_range < 1, goal_dim outside [1, state_dim], state_dim +
 * goal_dim != obs_dim, a mode outside the enum, a NaN tolerance, weights NULL with goal_dim != 3, L < 1, L + rows > capacity, a pick
 * outside [0, m_i); FRL_ERR_STATE: L > the learner's stored rows, a prioritised engine (the rows would bypass the priority trees),
 * an engine that is not FRL_ALGO_DDPG, FRL_ALGO_TD3 or FRL_ALGO_SAC. */
enum frl_her_mode { FRL_HER_SPARSE = 0, FRL_HER_SHAPING = 1 };
struct frl_her_args {
    int n_episodes;
    const int* learners;        /* host [n_episodes], each learner at most once */
    const int* lengths;         /* host [n_episodes]: L of each episode */
    int state_dim, goal_dim;
    int sample_num, sample_range;
    int mode;                   /* enum frl_her_mode */
    const double* weights;      /* host [goal_dim], or NULL: the script's 1, 1, 0.1 (goal_dim == 3 only) */
    double tolerance;           /* FRL_HER_SPARSE: the script's 0.5 */
    const float* env_actions;   /* host [sum L][act_dim], episode after episode: the action column block of the relabelled rows (the
                                   script stores the env-unit, noised, clipped action there, not the policy output of the real row);
                                   NULL: the stored action of transition i */
    const int32_t* picks;       /* host [sum rows], episode after episode in output order: the offset j - i in [0, m_i) of every
                                   row (for m_i < sample_num: 0, 1, ...); NULL: drawn on the device (Philox keyed by the engine's
                                   seed, the relabel call, the learner and i; uniform over the sample_num-subsets) */
    int* rows_out;              /* host [n_episodes] or NULL: the rows written per episode */
};
typedef struct frl_her_args frl_her_args;
int frl_her_relabel(frl_engine* e, const frl_her_args* args);

/* ---------------------------------------------------------------- parameters (state_dict)
 * Nets: DQN 0 = Qnet; DDPG/TD3/SAC/PPO 0 = actor, 1 = critic; MADDPG 2i = actor_i, 2i+1 = critic_i.
 * Flat layout = the reference state_dict tensors in layer order (l1.weight[out][in], l1.bias, l2...,
 * twin critic l1..l6), then log_std for Gaussian actors (DQN.py:131-138, SAC.py:274-282). */
int frl_net_count(const frl_engine* e, int* n_out);
int frl_net_num_params(const frl_engine* e, int net, int* n_out);
int frl_params_get(frl_engine* e, int learner, int net, int kind, float* out_host);
int frl_params_set(frl_engine* e, int learner, int net, int kind, const float* in_host);
/* invariant check: max |x| over the PADDING slots of one net's block of `kind` (weight rows / columns and bias entries past a
 * layer's real dims; layers are padded to multiples of 16).  The update kernels rely on the padding staying exactly zero — the
 * K-sliced first-layer sweeps read a record for 16 * ceil(in / 16) columns and let the zero weights cancel what lies past the
 * layer's inputs (which is why every field of a stored transition must be FINITE: 0 * inf is NaN; a non-finite value in a sampled
 * row poisons the reference's update as well, through the TD target) — and Adam keeps it: zero gradient, zero moments, zero step. */
int frl_params_pad_max(frl_engine* e, int learner, int net, int kind, float* max_abs_out);
int frl_opt_step_get(frl_engine* e, int learner, int net, int* t_out);   /* Adam step count */
int frl_opt_step_set(frl_engine* e, int learner, int net, int t);
/* SAC Alpha (SAC.py:154-169): vals = {log_alpha, exp_avg, exp_avg_sq, alpha} */
int frl_alpha_get(frl_engine* e, int learner, float* vals4_out, int* step_out);
int frl_alpha_set(frl_engine* e, int learner, const float* vals4, int step);
/* ... of ONE agent of a FRL_ALGO_MASAC engine (MASAC.py:124-139: one Alpha per agent), `step` its Adam step count.  On every other
 * engine agent must be 0 and the pair is frl_alpha_get / _set.  On a FRL_ALGO_MASAC engine with n_agents > 1 frl_alpha_get / _set
 * return FRL_ERR_STATE (there is no one alpha to name); with n_agents = 1 they serve agent 0. */
int frl_alpha_get_agent(frl_engine* e, int learner, int agent, float* vals4_out, int* step_out);
int frl_alpha_set_agent(frl_engine* e, int learner, int agent, const float* vals4, int step);

/* Batch_ObsNorm (`Normalization_batch_size`, PPO_file/normalization.py:53-84; SAC.py:181-182,215-217;
 * DDPG.py:160-161,190-192; PPO_with_tricks.py:225-226,297-299): when enabled, every learn call first
 * updates the running statistics with the batch mean of the sampled observations, then obs and
 * next_obs are normalised wherever the path reads them; select_action normalises without updating.
 * stats = {n, mean[O], S[O], std[O]}; a MADDPG engine (MADDPG.py:155-156,194-196) keeps one such block per agent, each 1 +
 * 3*max(obs_dim) floats wide, and get/set move all n_agents blocks. */
int frl_obsnorm_enable(frl_engine* e, int on);
int frl_obsnorm_get(frl_engine* e, int learner, float* stats_out);
int frl_obsnorm_set(frl_engine* e, int learner, const float* stats);

/* ---------------------------------------------------------------- forward (select_action)
 * in_host [P][n_rows][in_dim], eps_host [P][n_rows][out_dim] or NULL, out_host [P][n_rows][out_dim]
 * (ARGMAX: [P][n_rows] indices as float), logp_host like out or NULL.  Synchronous.
 * use_target: 0 online parameters, 1 target parameters, 2 the noisy net's effective set of the last frl_noisy_resample. */
int frl_act(frl_engine* e, int net, int mode, int head, int use_target, int n_rows, int in_dim, const float* in_host,
            const float* eps_host, float* out_host, float* logp_host);
/* same with DEVICE pointers, asynchronous on the engine stream (vectorised env pool path) */
int frl_act_device(frl_engine* e, int net, int mode, int head, int use_target, int n_rows, int in_dim,
                   const float* in_dev, const float* eps_dev, float* out_dev, float* logp_dev);

/* ---------------------------------------------------------------- learn (the hot path) */
int frl_learn(frl_engine* e, const frl_learn_args* args);
int frl_stats_get(frl_engine* e, float* out_host);          /* [P][n_agents][FRL_STAT_COUNT] */
/* the ring rows the last frl_learn trained on — `indices` of `<ALGO>.sample` (DQN.py:97): uploaded, device-drawn or (per = 1)
 * the last frl_per_sample's — as host int64 [P][n_agents][batch] */
int frl_last_indices(frl_engine* e, int batch, int64_t* out_host);
/* algorithmic work of one frl_learn launch (for the roofline figure): flops and HBM bytes, by SURVEY.md 8(d)'s formula —
 * 2 B sum(in x out) x (#forward + 2 x #backward passes), i.e. a dX is counted for every layer of every backward pass */
int frl_learn_work(const frl_engine* e, int batch, int do_actor, double* flops_out, double* bytes_out);
/* the same launch's EXECUTED flops: what torch autograd (and these kernels) actually compute — a trained net's backward is
 * dW for every layer but dX only from the second layer up (nothing needs d loss / d input), and the policy loss's pass through
 * the frozen critic (Q(s, pi(s)), TD3.py:225, SAC.py:245-249) is forward + dX with the first layer's dX on the agent's action
 * columns only.  8(d)'s figure is 1.6 % above this at the narrow bench shape and 30 % above it at config 4's 393-column first
 * layers; roofline fractions quote both, named. */
int frl_learn_work_executed(const frl_engine* e, int batch, int do_actor, double* flops_out);

/* ---------------------------------------------------------------- PPO (PPO_file/PPO_with_tricks.py)
 * `PPO.learn(minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient)` (:290-354):
 * value pass over the stored horizon, GAE scan, v_target, optional advantage normalisation, then
 * K_epochs x ceil(horizon/minibatch) actor + critic steps — three launches in total. */
typedef struct frl_ppo_args {
    int horizon;               /* rows 0..horizon-1 of the ring, in time order (Buffer_for_PPO.all, Buffer.py:312-323) */
    int minibatch, k_epochs;
    int adv_norm;              /* trick['adv_norm'] (:314-315) */
    float gamma, lmbda, clip, ent_coef;
    float actor_lr, critic_lr; /* per call so that PPO.lr_decay (:357-363) is the caller's arithmetic */
    float adam_eps;            /* 1e-5 with trick['adam_eps'] (:191-196) */
    float clip_norm;           /* 0.5 */
    int optimizer;             /* 0: torch.optim.Adam per net (PPO_with_tricks.py:191-196);
                                  1: PPO.py's combined cautious AdamW over actor + critic parameters (PPO.py:121,145-152,
                                     c_adamw.py:80-127): lr = actor_lr for both nets, eps = adam_eps (1e-6 there), mask =
                                     (exp_avg*grad > 0) / max(mean, 1e-3) PER PARAMETER TENSOR, no bias correction in denom */
    const int64_t* perms;      /* host [P][k_epochs][horizon] np.random.permutation draws (:320), or NULL: drawn on the device */
    float* loss_trace_out;     /* host [P][k_epochs*n_mb][2] (actor, critic) losses or NULL */
    float* adv_out;            /* host [P][horizon] raw GAE advantages or NULL */
    float* vtarget_out;        /* host [P][horizon] or NULL */
    int gae_mode;              /* 0: the value pass + TD-delta scan described above.
                                  1: PPO_advance/PPO_2.py:213-224 — no value pass: V(s_t) was stored at rollout time in the
                                     extra column before adv_done (Buffer_for_PPO_2.add, PPO_advance/Buffer.py:462-478) and
                                     the advantages / returns come from stable-baselines3's scan (:480-507) in float64:
                                     delta = r + gamma*next_value*(1-done) - V, A = delta + gamma*lambda*(1-adv_done)*A',
                                     returns = A + V, both cast to float32 once */
    const float* last_value;   /* gae_mode 1: host [P], the critic's value of the state after the last stored step */
    double gae_gamma, gae_lmbda; /* gae_mode 1: the scan's gamma / lambda as the caller's doubles (0: use gamma / lmbda) */
} frl_ppo_args;
int frl_ppo_learn(frl_engine* e, const frl_ppo_args* args);
/* ---------------------------------------------------------------- REINFORCE (REINFORCE_file/REINFORCE.py)
 * `REINFORCE.learn(gamma)` (:104-127) for every learner in one launch chain: the returns of the stored steps scanned backwards
 * (G = r + gamma G (1 - done), several episodes per call allowed, a truncated one carries G into the one before it), normalised
 * with the unbiased std, loss = sum_t -log pi(a_t|s_t) g_t with Categorical(probs)'s clamp at float32 eps, one Adam step, no
 * gradient clipping.  The stored steps are ring rows 0..n-1 in time order (frl_buffer_add* from an empty ring); a record's
 * next_obs columns are not read.  Afterwards the ring cursor of every learner that took part is (0, 0): the reference clearing its
 * lists.  FRL_STAT_ACTOR_LOSS is the loss, FRL_STAT_ACTOR_GNORM the gradient norm.
 * Refused before any launch: FRL_ERR_INVALID when a participating learner has exactly one step (torch.std of one element is NaN
 * and the reference turns every parameter into NaN) or more than `capacity`; FRL_ERR_STATE when its ring holds fewer rows than
 * asked for or was not filled from an empty cursor (index != size mod capacity: a wrapped ring is not in time order), and on
 * engines of any other algorithm.  frl_act serves this engine with FRL_ACT_RAW, FRL_ACT_ARGMAX and
 * FRL_ACT_CAT_SAMPLE; frl_learn, frl_ppo_learn, frl_rollout and frl_act_explore return FRL_ERR_STATE for it. */
struct frl_reinforce_args {
    const int* n_steps;   /* host [P]: learner p trains on ring rows 0..n_steps[p]-1, in time order; NULL: every learner's cursor size.
                             0: this learner sits the call out (nothing of its state changes) */
    double gamma;         /* the scan runs in float64, as the reference's Python floats do */
    float lr, adam_eps;
    float* loss_out;      /* host [P] or NULL (NULL: the call is asynchronous); entries of learners that sit out are left as they are */
    float* returns_out;   /* host [P][capacity] normalised returns or NULL; only rows 0..n_steps[p]-1 are written */
};
typedef struct frl_reinforce_args frl_reinforce_args;
int frl_reinforce_learn(frl_engine* e, const frl_reinforce_args* args);

/* ---------------------------------------------------------------- envelope multi-objective DQN (ENVELOPE_MORL_file/ENVELOPE_DQN.py)
 * `ENVELOPE.learn(batch_size, gamma, tau, weight_num, update_freq)` (:204-255) for every learner in one launch chain.  It trains on
 * N = batch x weight_num rows: row j is sampled ring row idx[j % batch] under preference weights[j / batch].  a' = argmax_a w . Q(s', w)[a]
 * of the ONLINE net (first maximum), T = r + gamma Q_target(s', w)[a'] (1 - done), Q = Q(s, w)[stored action], and
 *     loss = beta mean_j (w.Q - w.T)^2 + (1 - beta) mean_{j,k} (Q_k - T_k)^2
 * then one Adam step (torch defaults) WITHOUT gradient clipping (the reference's clip_grad_norm_ runs before backward() and clips
 * nothing) and the soft target update with `tau` on every call.  FRL_STAT_ACTOR_LOSS is the loss, FRL_STAT_ACTOR_GNORM the gradient
 * norm.  Refused before any launch with FRL_ERR_INVALID: batch < 1, weight_num < 1, batch x weight_num > batch_max, NaN scalars,
 * beta outside [0, 1]; with FRL_ERR_STATE: batch > a learner's stored rows, idx = NULL with fewer than 2 x batch stored rows, and
 * engines of any other algorithm.  frl_act serves this engine with FRL_ACT_RAW on in_dim = obs_dim + reward_dim; frl_learn,
 * frl_learn_path, frl_learn_work*, frl_rollout and frl_act_explore return FRL_ERR_STATE for it. */
struct frl_envelope_args {
    int batch;              /* B: sampled ring rows */
    int weight_num;         /* W: preference vectors; B x W <= batch_max */
    float gamma, tau, lr, beta;
    const int64_t* idx;     /* host [P][batch] rows drawn by the caller (ENVELOPE.sample, :191-200), or NULL: drawn uniformly on the device */
    const float* weights;   /* host [P][weight_num][reward_dim] preferences, used as given (:221-223), or NULL: |N(0,1)| / L1 norm on the device */
    float* loss_out;        /* host [P] or NULL (both outputs NULL: the call is asynchronous) */
    float* weights_out;     /* host [P][weight_num][reward_dim] or NULL: the preferences the call used */
};
typedef struct frl_envelope_args frl_envelope_args;
int frl_envelope_learn(frl_engine* e, const frl_envelope_args* args);

/* ---------------------------------------------------------------- envelope multi-objective DDPG (ENVELOPE_MORL_file/ENVELOPE_DDPG.py)
 * `ENVELOPE_DDPG.learn(batch_size, gamma, tau, weight_num, update_freq)` (:254-320) for every learner in one launch chain, on the
 * same N = batch x weight_num rows as frl_envelope_learn (row j: ring row idx[j % batch] under preference weights[j / batch]).
 * Critic step: a' = actor(s', w) of the ONLINE actor (:284), T = r + gamma critic_target(s', a', w) (1 - done), Q = critic(s, a, w),
 *     loss = beta mean_j (w.Q - w.T)^2 + (1 - beta) mean_{j,k} (Q_k - T_k)^2
 * clip_grad_norm_ at 0.5 (it runs after backward() here and clips), Adam with critic_lr.  Actor step through the updated critic:
 * loss = -mean_{j,k} critic(s, actor(s, w), w)_k (the objectives are NOT weighted by w), clip at 0.5, Adam with actor_lr.  Both
 * target nets then move by `tau`.  FRL_STAT_CRITIC_LOSS / _GNORM and FRL_STAT_ACTOR_LOSS / _GNORM hold the losses and the pre-clip
 * gradient norms.  Refusals are frl_envelope_learn's: FRL_ERR_INVALID for batch < 1, weight_num < 1, batch x weight_num > batch_max,
 * NaN scalars, beta outside [0, 1]; FRL_ERR_STATE for batch > a learner's stored rows, idx = NULL with fewer than 2 x batch stored
 * rows, and engines of any other algorithm.  frl_act serves this engine with FRL_ACT_TANHHEAD on net 0 (in_dim = obs_dim +
 * reward_dim) and FRL_ACT_RAW on net 1 (in_dim = obs_dim + act_dim + reward_dim); every other learn, rollout or explore entry
 * point returns FRL_ERR_STATE for it. */
struct frl_envelope_ddpg_args {
    int batch;              /* B: sampled ring rows */
    int weight_num;         /* W: preference vectors; B x W <= batch_max */
    float gamma, tau, actor_lr, critic_lr, beta;
    const int64_t* idx;     /* host [P][batch] rows drawn by the caller (ENVELOPE_DDPG.sample, :241-250), or NULL: drawn uniformly on the device */
    const float* weights;   /* host [P][weight_num][reward_dim] preferences, used as given (:269-271), or NULL: |N(0,1)| / L1 norm on the device */
    float* critic_loss_out; /* host [P] or NULL (all three outputs NULL: the call is asynchronous) */
    float* actor_loss_out;  /* host [P] or NULL */
    float* weights_out;     /* host [P][weight_num][reward_dim] or NULL: the preferences the call used */
};
typedef struct frl_envelope_ddpg_args frl_envelope_ddpg_args;
int frl_envelope_ddpg_learn(frl_engine* e, const frl_envelope_ddpg_args* args);

/* ---------------------------------------------------------------- GAIL's discriminator (GAIL_file/GAIL.py)
 * `GAIL.trian_D(expert_states, expert_actions, policy_states, policy_actions)` (:75-120) for every learner in one launch chain, on
 * E = n_expert expert rows (ring rows idx[j]: drawn WITH replacement, as InfiniteUniformSampler's torch.randint does) and
 * N = n_policy policy rows (uploaded).  With x = [s | a] and l the net's logit:
 *     gp = 0:  p = sigmoid(l);  d_loss = BCE(p_expert, 1) + BCE(p_policy, 0), each a mean over its own rows, with torch's clamps (both
 *              logs at -100, the backward's divisor max(p (1 - p), 1e-12)); the reference's Adam betas are (0.9, 0.999)
 *     gp = 1:  d_loss = 0.5 (mean_e softplus(-l) + mean_p softplus(l)) + gp_weight mean_e ||dl/dx||^2, the penalty on the EXPERT rows
 *              only and its weight the reference's literal 5 (NOT config gp_coef); the reference's betas are (0.5, 0.9)
 * then one Adam step with `lr`, the betas and eps given, no gradient clip, no target.  The penalty's gradient is second order; the
 * kernel takes it in closed form (csrc/device/gail.hpp), which needs a piecewise-linear hidden activation: frl_create refuses
 * FRL_ACT_TANH for this algorithm.  out[p] = { d_loss, mean p_expert (gp: mean sigmoid(l_expert)), mean p_policy, w_dis = mean l_expert -
 * mean l_policy (0 without gp), penalty mean (0 without gp), gradient norm }; FRL_STAT_ACTOR_LOSS / _GNORM hold d_loss and the norm.
 * Refused before any launch with FRL_ERR_INVALID: n_expert or n_policy < 1 or > batch_max, NaN scalars, betas outside [0, 1),
 * policy_rows NULL, gp outside {0, 1}, gp_weight < 0; with FRL_ERR_STATE: an idx entry at or past a learner's stored rows (negative
 * entries included), an empty ring, and engines of any other algorithm.  idx = NULL draws from the engine's Philox stream over the rows
 * EVERY learner's ring holds (the smallest ring's count).
 * frl_gail_reward is `GAIL.compute_reward` (:62-73) on n_rows uploaded rows per learner, fp32 in the reference's order of operations:
 *     gp = 1:  2 x -log(max(1 - 1 / (1 + exp(-l)), 1e-4));      gp = 0:  -log(1 - sigmoid(l) + 1e-8)
 * frl_act serves this engine with FRL_ACT_RAW on in_dim = obs_dim + act_dim (the logits, online net only); every other learn, rollout
 * or explore entry point returns FRL_ERR_STATE for it. */
struct frl_gail_args {
    int n_expert, n_policy;        /* E, N >= 1, each <= batch_max */
    int gp;                        /* 0: sigmoid + BCE; 1: logits, 0.5 x BCE-with-logits + gp_weight x penalty */
    float gp_weight;               /* the reference's literal 5 */
    float lr, beta1, beta2, adam_eps;
    const int64_t* idx;            /* host [P][n_expert] expert ring rows (torch.randint draws), or NULL: device draw with replacement */
    const float* policy_rows;      /* host [P][n_policy][obs_dim + act_dim] */
    float* out;                    /* host [P][6]: d_loss, expert_prob, policy_prob, w_dis (0 without gp), penalty mean (0 without gp), gradient norm; NULL: asynchronous */
    int64_t* idx_out;              /* host [P][n_expert] or NULL: the rows the call used */
};
typedef struct frl_gail_args frl_gail_args;
int frl_gail_learn(frl_engine* e, const frl_gail_args* args);
int frl_gail_reward(frl_engine* e, int gp, int n_rows, const float* rows_host /* [P][n_rows][obs_dim + act_dim] */, float* reward_out /* [P][n_rows] */);

/* ---------------------------------------------------------------- GAIL's policy side (GAIL_file/PPO2.py) on a FRL_ALGO_GAIL_PPO engine
 * `PPO.PPO_learn(batch, last_value)` (:235-307) for every learner in one launch chain over ring rows 0 .. horizon-1:
 *     V(s_t) and the old log-prob of the stored action under the actor BEFORE the update (summed over dimensions; the log-softmax entry
 *     for Categorical), both over the whole horizon;
 *     td_t = r_t + gamma V(s_{t+1}) - V(s_t) with V(s_{t+1}) the NEXT ROW's value also across an episode end (mask_1 == 1) and
 *     last_value[p] behind the last row;  A_t = td_t + c (1 - done_t) A_{t+1}, c = float32(double(gamma) * double(lam));
 *     returns = A + V;  A <- (A - mean) / (unbiased std + 1e-8);
 *     k_epochs x ceil(horizon / minibatch) steps: actor loss -mean(min(ratio A, clip(ratio, 1 -+ clip) A)) - ent_weight mean(entropy),
 *     critic loss value_loss_coef x mse(V, returns); each net clipped at global norm clip_norm on its own, then Adam (betas 0.9 / 0.999,
 *     eps 1e-8) with p_lr / v_lr; both nets count the same steps, as the reference's single optimiser does.  A last minibatch shorter than
 *     `minibatch` is averaged over its own size.
 * r_t is the ring's reward column, or rewards[p][t] when `rewards` is given (the discriminator's).  The call does NOT reset the ring's
 * cursors (the reference clears its memory in the loop): frl_buffer_cursor_set does.
 * Refused before any launch with FRL_ERR_INVALID: horizon < 2 (the unbiased std of one row is NaN) or > capacity, minibatch < 1 or
 * > batch_max, k_epochs < 1, a permutation entry outside [0, horizon); with FRL_ERR_STATE: engines of any other algorithm.  frl_learn,
 * frl_ppo_learn, the rollout and explore entry points return FRL_ERR_STATE for a FRL_ALGO_GAIL_PPO engine. */
struct frl_gail_ppo_args {
    int horizon, minibatch, k_epochs;
    float gamma, lam, clip, ent_weight, value_loss_coef;
    float p_lr, v_lr, clip_norm;   /* clip_norm: the reference's literal 0.5 (<= 0: no clipping) */
    const float* last_value;       /* host [P] V of the state behind the last row, or NULL: 0 */
    const float* rewards;          /* host [P][horizon] replacing the ring's reward column, or NULL */
    const int64_t* perms;          /* host [P][k_epochs][horizon] torch.randperm draws, or NULL: drawn on the device */
    float* adv_out;                /* host [P][horizon] advantages BEFORE normalisation, or NULL */
    float* returns_out;            /* host [P][horizon], or NULL */
    float* logp_old_out;           /* host [P][horizon], or NULL */
    float* loss_trace_out;         /* host [P][k_epochs * ceil(horizon / minibatch)][2] (actor, critic) loss of every step, or NULL */
};
typedef struct frl_gail_ppo_args frl_gail_ppo_args;
int frl_gail_ppo_learn(frl_engine* e, const frl_gail_ppo_args* args);
/* The clamp range of the actor's log_std on a FRL_ALGO_GAIL_PPO engine (config['PPO']['log_std_min' / 'log_std_max']): read by the
 * update kernels (closed-bound gradient gate, as torch.clamp) and by frl_act's FRL_ACT_PPO_SAMPLE.  FRL_ERR_INVALID unless lo < hi and
 * both are finite; FRL_ERR_STATE on engines of any other algorithm (theirs is compiled in: [-20, 2]). */
int frl_log_std_range_set(frl_engine* e, float lo, float hi);
int frl_log_std_range_get(const frl_engine* e, float* lo_out, float* hi_out);

/* ---------------------------------------------------------------- CEM_GD3PG (CEM_GD3PG_file/CEM_GD3PG.py) on a FRL_ALGO_CEM_GD3PG engine
 * The two rings of a learner.  Ring 0 is `buffer`, ring 1 `buffer_domain` (:134-135); each has `capacity` rows, its own cursor and size,
 * and Buffer.add's arithmetic (index = (index + 1) % capacity, size = min(size + 1, capacity)).  Engines of every other algorithm have
 * ring 0 only, where these are frl_buffer_add / _add_batch / _cursor_get / _cursor_set; FRL_ERR_INVALID for a ring the engine lacks. */
int frl_ring_add(frl_engine* e, int learner, int ring, const float* record);
int frl_ring_add_batch(frl_engine* e, int ring, int n, const int* learners /* [n] or NULL: learner 0 */, const float* records /* [n][width] */);
int frl_ring_cursor_get(const frl_engine* e, int learner, int ring, int* index_out, int* size_out);
int frl_ring_cursor_set(frl_engine* e, int learner, int ring, int index, int size);
/* `CEM_GD3PG.learn(batch_size, gamma, tau, is_F1_more, delta, actor_domain)` (:180-231) for every learner in one launch chain over
 * B = 2 half rows, half = min(len(buffer_domain), batch) / 2 (:160-176; the smallest ring 1 of the population decides): `half` rows of
 * ring 0, then `half` rows of ring 1, BOTH drawn below ring 1's size — rows of ring 0 that were never written read as zeros, as the
 * reference's do.
 *   Critic step: T = r + gamma (1 - done) min(critic_target(s', actor_1_target(s')), critic_target(s', actor_2_target(s'))), MSE against
 *     critic(s, a), clip_grad_norm_ 0.5, Adam(critic_lr).
 *   Actor steps, through the critic just stepped: the unguided actor u (actor_1 if f1_more, else actor_2) has loss -mean Q(s, actor_u(s));
 *     the guided actor g, the other one, has -mean Q(s, actor_g(s)) + lambda delta KL with c = actor_g(s) - actor_domain(s) and
 *     KL = sqrt(sum c^2 / B).  Each has its own clip at 0.5 and Adam(actor_lr).  sum c^2 == 0 (torch: NaN gradients): the penalty's gradient
 *     is taken as 0 and KL is reported as 0.
 *   Soft update of the three targets with tau.  Net 3 (actor_domain) is read only.
 * Refused before any launch with FRL_ERR_INVALID: batch < 2, 2 half > batch_max, NaN scalars or a NaN delta, f1_more / delta NULL, an idx
 * entry outside [0, capacity) (ring 0: what was never written is zeros) or outside [0, size of ring 1) (ring 1); with FRL_ERR_STATE: a
 * ring 1 that holds fewer than 2 rows, and engines of any other algorithm.  Every other learn, rollout or explore entry point returns
 * FRL_ERR_STATE for a FRL_ALGO_CEM_GD3PG engine and names this one. */
struct frl_cem_gd3pg_args {
    int batch;              /* batch_size */
    float gamma, tau, actor_lr, critic_lr;
    float lambda;           /* Actor.lambda_ (:42): 10 */
    const int* f1_more;     /* host [P]: is_F1_more of every learner (nonzero: actor_1 is unguided, actor_2 guided) */
    const float* delta;     /* host [P] */
    const int64_t* idx;     /* host [P][2][half] ring-relative rows, ring 0's first (the two np.random.choice draws, :165-166), or NULL:
                               drawn on the device without replacement, both halves below ring 1's size */
    float* out;             /* host [P][8] = {critic loss, critic pre-clip norm, actor_1 loss, actor_1 norm, actor_2 loss, actor_2 norm,
                               KL, rows used} or NULL: the call is asynchronous.  FRL_STAT_CRITIC_LOSS / _CRITIC_GNORM / _ACTOR_LOSS /
                               _ACTOR_GNORM (actor_1's) carry the same values */
};
typedef struct frl_cem_gd3pg_args frl_cem_gd3pg_args;
int frl_cem_gd3pg_learn(frl_engine* e, const frl_cem_gd3pg_args* args);

/* ---------------------------------------------------------------- MAPPO / IPPO (MAPPO_file/MAPPO.py, IPPO.py)
 * `MAPPO.learn / IPPO.learn(minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta)` for every learner in
 * one launch chain: every critic's V(s), V(s') over the horizon, the GAE scan per agent (float32) from that agent's reward, done and
 * adv_done columns, v_target = adv + V(s), the optional advantage normalisation, then k_epochs x ceil(horizon / minibatch) steps of
 * every agent's actor and critic.  What the two engine kinds do differently, as the reference's two files do:
 *     IPPO   the critic reads the agent's own observation; actor and critic of agent i use column i of adv / v_target; adv_norm is
 *            per column (std over horizon - 1)
 *     MAPPO  the critic reads every agent's observation; the surrogate of EVERY actor is the mean over all n_agents advantage columns
 *            (ratios [m, 1] x adv[index] [m, n]) and EVERY critic regresses V repeated n times on all n target columns; adv_norm is
 *            over the whole [horizon, n_agents] matrix (std over horizon x n_agents - 1)
 * MAPPO.py's one Adam over actor + critic parameters (lr = actor_lr, eps 1e-5, no gradient clip) is elementwise, hence two Adams with
 * equal settings: its caller passes critic_lr = actor_lr, adam_eps = 1e-5, clip_norm = 0.  value_clip is accepted and changes nothing:
 * the reference clamps the TARGET around V and takes torch.max of the two MEAN losses, which always steps like, and reports, the
 * unclipped loss (DESIGN.md "MAPPO / IPPO" has the argument).  Afterwards every ring cursor is (0, 0): Buffer_for_PPO.clear.
 * Refused before any launch with FRL_ERR_INVALID: horizon outside [2, capacity], minibatch outside [1, batch_max], k_epochs < 1, a
 * loss_kind other than FRL_LOSS_MSE / FRL_LOSS_HUBER, FRL_LOSS_HUBER with huber_delta <= 0, a permutation entry outside [0, horizon),
 * minibatch != horizon on an engine with a state block and FRL_STATE_ROWS_POSITION (frl_create_ex);
 * with FRL_ERR_STATE: engines of any other algorithm (FRL_ALGO_HAPPO among them: frl_happo_learn).  frl_act serves these engines with FRL_ACT_RAW (the critic's value on nets
 * 2i+1; a MAPPO critic's input row is [obs_0 | ... | obs_{n-1}], and [obs_0 | ... | obs_{n-1} | state], in_dim = sum obs_dim +
 * state_dim, on an engine with a state block: frl_create_ex), FRL_ACT_TANHHEAD, FRL_ACT_ARGMAX, FRL_ACT_PPO_SAMPLE and
 * FRL_ACT_CAT_SAMPLE, through the same normalised forward as the update; every other learn, rollout or explore entry point returns
 * FRL_ERR_STATE for them. */
struct frl_mappo_args {
    int horizon;               /* rows 0..horizon-1 of the ring, in time order */
    int minibatch, k_epochs;
    float gamma, lmbda, clip, ent_coef;
    float actor_lr, critic_lr; /* per call, so that lr_decay is the caller's arithmetic */
    float adam_eps;            /* IPPO: 1e-5 with trick['adam_eps'], else 1e-8 (0 means 1e-8); MAPPO: 1e-5 */
    float clip_norm;           /* IPPO: 0.5; <= 0: none (MAPPO) */
    int adv_norm;              /* trick['adv_norm'] */
    int value_clip;            /* trick['ValueClip']: accepted, without effect (above) */
    int loss_kind;             /* FRL_LOSS_MSE, or FRL_LOSS_HUBER with trick['huber_loss'] */
    float huber_delta;         /* the scripts' 10 */
    const int64_t* perms;      /* host [P][n_agents][k_epochs][horizon] np.random.permutation draws in the reference's order (agent-major), or
                                  NULL: drawn on the device */
    float* adv_out;            /* host [P][horizon][n_agents] advantages before normalisation, or NULL */
    float* vtarget_out;        /* host [P][horizon][n_agents] or NULL */
    float* loss_trace_out;     /* host [P][n_agents][k_epochs * n_mb][2] (actor, critic) loss of every step, or NULL */
};
typedef struct frl_mappo_args frl_mappo_args;
int frl_mappo_learn(frl_engine* e, const frl_mappo_args* args);
/* trick['feature_norm'] / trick['LayerNorm'] of a MAPPO / IPPO engine: F.layer_norm (no affine part, biased variance, eps 1e-5) over the
 * whole input row before l1, and over the hidden row after each ReLU, in every net of the engine and in every forward (frl_act and
 * frl_mappo_learn alike).  Both are off at create (MAPPO_simple / IPPO_simple); the LDS of the LayerNorm case is reserved at create,
 * so the call cannot fail for space.  Engines of any other algorithm return FRL_ERR_STATE. */
int frl_net_norm_set(frl_engine* e, int feature_norm, int layer_norm);
/* Invalid-action masking (MAPPO_file/MAPPO_for_mask_action.py) on a discrete FRL_ALGO_MAPPO engine created with
 *     extra_cols = n_agents (log-probs) + n_agents (adv_done) + sum_i act_dim[i]
 * so that a record's extra columns are [log-probs | adv_done x n | mask block of agent 0 | .. | mask block of agent n-1], block i being
 * act_dim[i] floats, nonzero = the action is available.  on != 0: frl_mappo_learn reads the masks: the actor's row becomes
 * CategoricalMasked, i.e. Categorical(logits = where(mask, logits, -1e8)), normalised in torch's order l = logits' - (max + log sum
 * exp(logits' - max)) (a row whose mask is all closed has l = 0 everywhere: log-prob 0, no entropy, no gradient), entropy = -sum over
 * the open actions of p l, no gradient into a closed action, the log-prob not clamped.  The critic, GAE, v_target and adv_norm are
 * FRL_ALGO_MAPPO's; the caller passes the reference's two Adams as for IPPO (two lrs, clip_norm 0.5).  The reference's learn() runs on
 * the WHOLE capacity in one minibatch whatever the cursor says (Buffer_for_PPO_mask.all()): pass horizon = minibatch = capacity; rows
 * never written read as zeros (frl_create zeroes the ring) and rows of earlier episodes stay (clear() resets the counters only).
 * on == 0: masking off, the blocks are ignored.  FRL_ERR_STATE on any engine but FRL_ALGO_MAPPO (IPPO and HAPPO engines too);
 * FRL_ERR_INVALID when the engine's actions are continuous or its extra_cols hold no mask blocks (on an engine with a state block,
 * frl_create_ex: no mask blocks in front of that block).  A refused call changes nothing. */
int frl_action_mask_set(frl_engine* e, int on);
/* select_action of such an engine: for every learner and row, CategoricalMasked(logits = actor `net`(in), masks = mask).sample() and
 * its log_prob.  in_host [P][n_rows][in_dim]; mask_host [P][n_rows][act_dim], nonzero = available; eps_host [P][n_rows][act_dim]
 * Exp(1) draws (torch's `empty_like(p).exponential_(1)`: the sample is argmax(p / q)), or NULL: drawn on the device; out_host
 * [P][n_rows] the action index; logp_host [P][n_rows] its normalised logit, or NULL.  A closed action has p = 0 and is never drawn
 * while any is open.  Synchronous.  FRL_ERR_STATE unless masking is on for the engine; FRL_ERR_INVALID for a net that is not an actor
 * (even index), in_dim other than its input width, NULL in / mask / out or n_rows < 1. */
int frl_act_masked(frl_engine* e, int net, int n_rows, int in_dim, const float* in_host, const float* mask_host, const float* eps_host,
                   float* out_host, float* logp_host);

/* ---------------------------------------------------------------- HAPPO (MAPPO_file/HAPPO.py)
 * `HAPPO.learn(minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta)` for every learner.  Values, the
 * GAE scan, v_target and adv_norm over the whole [horizon, n_agents] matrix are FRL_ALGO_MAPPO's (HAPPO.py:343-370), and so are the
 * surrogate's mean over all n_agents advantage columns, the critic's regression of V repeated n times on all n target columns
 * (:420-440) and the ValueClip that changes nothing.  What HAPPO adds (:373-453): factor = ones [horizon]; the agents are visited in
 * the order `agent_order`; the visited agent's actor and critic take their k_epochs x ceil(horizon / minibatch) steps, the actor on
 *     -(factor[idx] * min(surr1, surr2)).mean() - ent_coef * entropy.mean()          (the entropy term is not weighted)
 * and unless it is the last visited, factor *= exp(new - old) row by row, with old / new = sum_c log pi(a | o) of that actor over the
 * whole horizon before / after its steps (float32, no clamp).  Each agent has two Adams (:237-254): the caller passes its two learning
 * rates, adam_eps 1e-5 with trick['adam_eps'] else 1e-8, clip_norm 0.5.  One launch per visiting position follows the three advantage
 * launches on the engine's one stream; stream order alone carries the dependency between agents.
 * Deviation from the reference, discrete actions only: HAPPO.py:449-450 takes `new` on `[index]`, the LAST MINIBATCH of the epoch loop,
 * against `old` over all rows - a RuntimeError unless that minibatch has horizon rows (then in permuted order against time order) or
 * one row (a silent broadcast).  Here both kinds do what the continuous branch does: all rows, in time order (DESIGN.md "HAPPO").
 * Refusals are frl_mappo_learn's, and FRL_ERR_INVALID before any launch for an agent_order row that is not a permutation of
 * 0..n_agents-1; FRL_ERR_STATE on engines of any other algorithm, and frl_mappo_learn returns it for FRL_ALGO_HAPPO engines.  A refused
 * call changes nothing and does not clear the ring; afterwards every ring cursor is (0, 0).  frl_net_norm_set and frl_act serve these
 * engines as they serve FRL_ALGO_MAPPO engines; every other learn, rollout or explore entry point returns FRL_ERR_STATE. */
struct frl_happo_args {
    /* frl_mappo_args' fields, in its order and with its meaning; perms and loss_trace_out are indexed by AGENT ID, not by visiting position */
    int horizon;
    int minibatch, k_epochs;
    float gamma, lmbda, clip, ent_coef;
    float actor_lr, critic_lr;
    float adam_eps;            /* 1e-5 with trick['adam_eps'], else 1e-8 (0 means 1e-8) */
    float clip_norm;           /* 0.5 */
    int adv_norm;
    int value_clip;
    int loss_kind;
    float huber_delta;
    const int64_t* perms;      /* host [P][n_agents][k_epochs][horizon], or NULL: drawn on the device.  The reference draws them while it
                                  visits: the k_epochs permutations of the first VISITED agent first */
    float* adv_out;
    float* vtarget_out;
    float* loss_trace_out;
    /* HAPPO's own */
    const int32_t* agent_order;/* host [P][n_agents]: the agent visited at each position (torch.randperm(n_agents), HAPPO.py:375), or NULL:
                                  a Fisher-Yates shuffle per learner on the host from the engine's seed and call counter */
    float* factor_out;         /* host [P][n_agents][horizon] BY VISITING POSITION: the factor the k-th visited agent's steps used; slice 0
                                  is all ones.  Or NULL */
};
typedef struct frl_happo_args frl_happo_args;
int frl_happo_learn(frl_engine* e, const frl_happo_args* args);

/* stand-alone GAE scan (K3) on device arrays [n_seq][horizon]: replaces the host loop at
 * PPO_with_tricks.py:308-311 / PPO.py:229-231 */
int frl_gae(frl_engine* e, const float* td_delta_dev, const float* adv_done_dev, int n_seq, int horizon,
            float gamma, float lmbda, float* adv_out_dev);

/* floats of factorised noise ONE forward of a noisy net consumes (0 for other engines) */
int frl_noisy_eps_size(const frl_engine* e, int* n_out);
/* one forward's worth of fresh noise for select_action (DQN_with_tricks.py:213-216 through Noisy_net.py:41-44): eps_host
 * [P][frl_noisy_eps_size] or NULL (device draw); afterwards frl_act(..., use_target = 2, ...) runs the net with it */
int frl_noisy_resample(frl_engine* e, const float* eps_host);

/* ---------------------------------------------------------------- prioritised replay
 * PER_Buffer + SumTree (DQN_file/Buffer.py:66-194) on the engine's ring: a float64 sum-tree and max-tree per learner in HBM.
 * add (frl_buffer_add*) gives new rows the current maximum priority, 1.0 on an empty buffer (:92-98). */
/* PER_Buffer.__init__ (:81-90).  beta and its increment stay doubles (the reference's Python floats); alpha and epsilon act
 * on float32 TD errors. */
int frl_per_enable(frl_engine* e, double alpha, double beta, double beta_increment, double epsilon);
/* PER_Buffer.sample (:99-124): beta += increment; `batch` stratified descents with s = a + (b-a)*u.  uniforms: host
 * [P][batch] draws of np.random.uniform's underlying random_sample(), or NULL (device Philox).  The sampled rows become the
 * engine's current sample (frl_learn with per = 1); idx_out / is_weight_out: host [P][batch] or NULL. */
int frl_per_sample(frl_engine* e, int batch, const double* uniforms, int64_t* idx_out, float* is_weight_out);
/* PER_Buffer.update_priorities (:126-129): priority = (|td| + epsilon)^alpha in float32.  idx / td_error: host [P][batch],
 * or NULL = the rows of the last frl_per_sample / the TD errors the last frl_learn(per = 1) left on the device. */
int frl_per_update(frl_engine* e, int batch, const int64_t* idx, const float* td_error);
int frl_per_state(frl_engine* e, int learner, double* sum_out, double* max_out, double* beta_out);   /* sumtree.sum(), .max(), beta */

/* ---------------------------------------------------------------- env pool + rollout
 * The step BEFORE the path: the reference steps one Python env inline per update (DQN.py:316) and
 * pays H2D + D2H per step in select_action (DQN.py:77,83).  The pool steps n env instances on
 * host worker threads into pinned staging; frl_rollout runs the whole per-step order of the
 * reference loop (select_action -> exploration -> env.step -> add -> learn; DQN.py:294-339,
 * TD3.py:403-450) for P learners x E instances per launch chain. */
enum frl_env_kind { FRL_ENV_PENDULUM = 0, FRL_ENV_CARTPOLE = 1, FRL_ENV_SYNLINEAR = 2, FRL_ENV_SYNLINEAR_DISCRETE = 3,
                    FRL_ENV_PENDULUM_SHORT = 4,
                    FRL_ENV_SYNBAND_WIDE = 5 /* obs 376 / act 17 (Humanoid-v4's dims, SAC.py:519-576 at BASELINE config 4) on banded
                                                linear dynamics: sizes the rollout path, not the physics */ };
typedef struct frl_envpool frl_envpool;
/* params: optional SynLinear matrices A[8][8] then B[8][2] (doubles), else NULL */
int frl_envpool_create(int kind, int n_envs, int n_threads, uint64_t seed, const double* params, int n_params,
                       frl_envpool** out);
/* A pool over caller-supplied environments (the gymnasium protocol the reference's loops drive, DQN.py:292,316: reset() ->
 * obs, step(a) -> obs, reward, terminated, truncated): ONE vectorised callback steps all n envs into the pool's pinned
 * staging and resets the finished ones (obs_next = the reset observation, like the built-in kinds).  Return 0 on success.
 * n_actions > 0: discrete (actions = [n] indices as float, act_dim 1). */
typedef int (*frl_env_step_fn)(void* user, const float* actions, float* next_obs, float* reward, uint8_t* terminated,
                               uint8_t* truncated, float* obs_next);
typedef int (*frl_env_reset_fn)(void* user, float* obs_out);
int frl_envpool_create_callback(int n_envs, int obs_dim, int act_dim, int n_actions, float max_action, frl_env_step_fn step,
                                frl_env_reset_fn reset, void* user, frl_envpool** out);
int frl_envpool_destroy(frl_envpool* p);
int frl_envpool_dims(const frl_envpool* p, int* n_envs, int* obs_dim, int* act_dim, int* n_actions, float* max_action,
                     int* max_steps);
int frl_envpool_reset(frl_envpool* p, float* obs_out);                       /* host [n][obs_dim] */
int frl_envpool_set_state(frl_envpool* p, int env, const double* state);     /* test hook: physical state of one env */
/* actions host [n][act_dim] in env units (discrete: [n] indices as float); outputs host arrays:
 * next_obs = observation of the transition, obs_next = what the policy sees next (reset obs after a done) */
int frl_envpool_step(frl_envpool* p, const float* actions, float* next_obs, float* reward, uint8_t* terminated,
                     uint8_t* truncated, float* obs_next);
/* The reference loops' per-step exploration rules, applied INSIDE the act launch from the engine's Philox stream (the
 * reference draws them from NumPy's global generator on the host, one env at a time):
 *   EPS_GREEDY  DQN.py:307-310    np.random.rand() < epsilon -> np.random.randint(action_dim), else the greedy action
 *   GAUSS       TD3.py:412        action_ = clip(a*max_action + scale * N(0, sigma*max_action), +-max_action)
 *   OU          SAC.py:334-356,529  x += theta*(0 - x) + sqrt(dt)*sigma*N(0,1); action_ = clip(a*max_action + x*scale*max_action)
 *   NONE        SAC.py:533, PPO_with_tricks.py:529-530  action_ = clip(a*max_action)
 * The action handed to add() is the policy's own output (continuous) or the explored index (discrete), as in the reference. */
enum frl_explore_kind { FRL_EXPLORE_NONE = 0, FRL_EXPLORE_EPS_GREEDY = 1, FRL_EXPLORE_GAUSS = 2, FRL_EXPLORE_OU = 3,
                        FRL_EXPLORE_OFF = 4 /* frl_rollout_args.explore_kind only: explicitly no exploration noise */ };
/* frl_rollout_args.explore_kind counts 0 differently from frl_explore_args.kind (since frl_version 101): there 0 is what a
 * zero-initialised struct carries and selects the algorithm's loop default, so "no noise" has its own value, FRL_EXPLORE_OFF.
 * Write FRL_EXPLORE_DEFAULT, never FRL_EXPLORE_NONE, into rollout args; frl_act_explore rejects FRL_EXPLORE_OFF. */
#define FRL_EXPLORE_DEFAULT 0
typedef struct frl_explore_args {
    int kind;
    float epsilon;
    float sigma;              /* gauss_sigma */
    float scale;              /* gauss_scale / OUNoise.scale (1 = none) */
    float max_action;
    float ou_theta, ou_sigma, ou_dt;
} frl_explore_args;
/* obs host [P][n_rows][obs_dim]; ended host [P][n_rows] or NULL (1: reset that row's OU state first, SAC.py:546-547);
 * outputs host [P][n_rows][act_dim] (FRL_ACT_ARGMAX: [P][n_rows]): the action add() stores, and the env-unit action. */
int frl_act_explore(frl_engine* e, int mode, int n_rows, const float* obs_host, const frl_explore_args* x,
                    const uint8_t* ended_host, float* store_act_out, float* env_act_out);

typedef struct frl_rollout_args {
    int n_steps;             /* vector steps (each steps every env once) */
    int envs_per_learner;    /* E; the pool must hold P*E envs, env i feeds learner i/E */
    int start_steps;         /* learn once every ring holds more rows than this (`step > start_steps`) */
    int learn_every;         /* vector steps per frl_learn call; 0: collect only */
    int policy_freq;         /* TD3 delayed actor update (TD3.py:224) */
    float epsilon;           /* DQN epsilon-greedy (DQN.py:307) */
    float explore_sigma;     /* Gaussian action-noise std as a fraction of max_action (gauss_scale*gauss_sigma, TD3.py:412) */
    frl_learn_args learn;    /* idx / noise / stats_out must be NULL; per = 1|2 (PER engines): frl_per_sample / frl_per_update around every learn */
    int host_explore;        /* 0: exploration inside the act launch — per vector step ONE D2H (env actions) and ONE H2D (the
                              * env outputs), records assembled on the device; 1: round 1's loop (host generator, obs H2D +
                              * action D2H + staged records H2D) kept for comparison */
    int explore_kind;        /* FRL_EXPLORE_DEFAULT (0, a zero-initialised struct) or -1: the algorithm's loop default (DQN
                              * epsilon-greedy, DDPG/TD3 Gaussian, SAC none); FRL_EXPLORE_EPS_GREEDY / _GAUSS / _OU: that rule;
                              * FRL_EXPLORE_OFF: none (a deterministic evaluation rollout).  NOT FRL_EXPLORE_NONE: that is 0 */
    float gauss_init_scale, gauss_final_scale;   /* with max_episodes > 0: a learner's noise multiplier decays with ITS finished episodes, */
    int max_episodes;                            /* scale = final + (init - final) * max(0, max_episodes - episodes) / max_episodes (TD3.py:425-427, SAC.py:548-556) */
    float ou_theta, ou_sigma, ou_dt;             /* OUNoise(theta 0.15, sigma, dt) (SAC.py:334-356) */
} frl_rollout_args;
typedef struct frl_rollout_stats {
    long long env_steps, updates, episodes;
    double return_sum, seconds;
} frl_rollout_stats;
int frl_rollout(frl_engine* e, frl_envpool* p, const frl_rollout_args* args, frl_rollout_stats* out);
/* On-policy counterpart for PPO engines (BASELINE config 3, PPO with vectorised envs): the reference steps one env for
 * `horizon` steps and calls learn() (PPO_with_tricks.py:524-569); here every learner steps E env instances for
 * horizon / E vector steps per cycle — select_action (:234-255) batched over all envs, action_ = clip(action *
 * max_action) (:529-530), add(obs, action, reward, next_obs, terminated, log_pi, terminated or truncated) (:541-545) —
 * then frl_ppo_learn.  Env j's steps fill ring rows [j*steps_per_env, (j+1)*steps_per_env); the last row of each
 * segment is marked adv_done so that the GAE scan restarts there as it does at the end of the reference's horizon.
 * stats: updates = minibatch steps (one actor + one critic step each). */
typedef struct frl_ppo_rollout_args {
    int n_iters;             /* collect + learn cycles */
    int envs_per_learner;    /* E; the pool must hold P*E envs */
    int steps_per_env;       /* vector steps per cycle; learn.horizon must equal E * steps_per_env */
    frl_ppo_args learn;      /* perms / outputs NULL (device-side permutations), gae_mode 0 */
} frl_ppo_rollout_args;
int frl_ppo_rollout(frl_engine* e, frl_envpool* p, const frl_ppo_rollout_args* args, frl_rollout_stats* out);

/* Algorithmic flops / bytes of one frl_ppo_learn over all learners (the figure a PPO roofline fraction is computed from). */
int frl_ppo_work(const frl_engine* e, int horizon, int k_epochs, double* flops_out, double* bytes_out);

/* ---------------------------------------------------------------- multi-GPU: the path's ONE collective
 * The reference is single-process / single-device and has no distributed code (its only trace is the dead import
 * DDPG_file/misc(lose).py:4): independent seeds / env-instance sets are sharded one process per GPU and nothing on the data
 * path is exchanged.  What IS exchanged is a short metrics vector per reporting interval — counters summed, wall-clock maxed —
 * by ncclAllReduce over RCCL (xGMI inside a node).  Bootstrap like NCCL's: ONE rank calls frl_comm_unique_id and ships the
 * 128 bytes to the others by any host channel (freerl_amd/dist.py: the launcher's store); every rank then calls
 * frl_comm_create collectively.  RCCL is bound at run time (dlopen), so the library loads on a box without it. */
#define FRL_COMM_ID_BYTES 128
#define FRL_COMM_MAX_VALUES 64
typedef struct frl_comm frl_comm;
int frl_comm_unique_id(uint8_t* id_out /* [FRL_COMM_ID_BYTES] */);
int frl_comm_create(const uint8_t* id, int rank, int world, int device_id, frl_comm** out);
int frl_comm_destroy(frl_comm* c);
int frl_comm_info(const frl_comm* c, int* rank_out, int* world_out);      /* NULL comm: rank 0 of 1 */
/* sums[n_sum] <- sum over ranks, maxes[n_max] <- max over ranks, in place (float64: counters exact to 2^53); at most
 * FRL_COMM_MAX_VALUES each.  comm == NULL: the single-process case, the vectors are already the job's totals.  Synchronous. */
int frl_metrics_allreduce(frl_comm* c, double* sums, int n_sum, double* maxes, int n_max);

/* developer read-back of the single-learner kernels' per-workgroup block (partial sums; section stamps in a timing build):
 * [16][32] floats of learner 0 (tools/solo_timing.py) */
int frl_solo_debug_read(frl_engine* e, float* out_host, int n_floats);

/* ---------------------------------------------------------------- timing on the engine stream */
int frl_timer_start(frl_engine* e);
int frl_timer_stop(frl_engine* e, float* ms_out);           /* synchronises */
/* per-kernel durations of frl_learn's launch chain (HIP events around every launch while enabled):
 * slots 0 draw, 1 grad(critic/Q), 2 adam(critic/Q), 3 grad(actor), 4 adam(actor), 5 soft update */
int frl_profile_enable(frl_engine* e, int on);
int frl_profile_read(frl_engine* e, double* ms_sum8_out, long long* count8_out);

#ifdef __cplusplus
}
#endif
#endif /* FREERL_HIP_H */
