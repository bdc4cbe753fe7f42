// Env pool + rollout collector entry points (included at the end of frl_api.hip).
#include "envpool.hpp"

struct frl_envpool {
    HostMem mem;                // owns the pinned and device buffers below (envpool_bind allocates, envpool_free_buffers releases)
    frl::EnvPool* pool = nullptr;
    // pinned staging (allocated lazily by frl_rollout on the engine's device)
    float* obs = nullptr;       // [n][O] what the policy sees
    float* next_obs = nullptr;  // [n][O] terminal observation of the last transition
    float* obs_next = nullptr;  // [n][O] observation after auto-reset
    float* act_out = nullptr;   // [n][Aout] policy output (D2H)
    float* eps = nullptr;       // [n][A] N(0,1) for stochastic policies (H2D)
    float* env_act = nullptr;   // [n][A] env-unit actions
    float* reward = nullptr;
    uint8_t* term = nullptr;
    uint8_t* trunc = nullptr;
    float* d_obs = nullptr;
    float* d_out = nullptr;
    float* d_eps = nullptr;
    float* logp = nullptr;      // [n][A] per-dimension log-probabilities of the sampled actions (PPO collector, D2H)
    float* d_logp = nullptr;
    bool pinned = false, started = false;
    frl::XorShift host_rng;
    long long total_it = 0;
    // ---- device-side exploration path (frl_rollout with host_explore = 0, frl_ppo_rollout): per vector step ONE D2H
    // (env actions) and ONE H2D (this block), the records are assembled on the device (replay_commit_kernel)
    unsigned char* blk = nullptr;      // pinned: [scale P f32 | row n i32 | next_obs n*O | obs_next n*O | reward n | flags n u8]
    unsigned char* d_blk = nullptr;
    size_t blk_bytes = 0, off_row = 0, off_nobs = 0, off_onext = 0, off_rew = 0, off_flags = 0;
    float* d_obs_cur = nullptr;        // [n][O] what the policy sees at the next act launch
    float* d_store = nullptr;          // [n][aout] the action add() stores
    float* d_env = nullptr;            // [n][A] env-unit actions (D2H -> env_act)
    float* d_ou = nullptr;             // [n][A] Ornstein-Uhlenbeck state
    int* done_flag = nullptr;          // pinned: the folded DQN step's launch writes its sequence number here once the actions are out
    int done_seq = 0;
    int* go_flag = nullptr;            // pinned: the doorbell of a pre-armed launch (the host writes the launch's go value once the step's block is filled)
    int go_seq = 0;
    hipStream_t stream2 = nullptr;     // the pre-armed launches alternate between the engine's stream and this one (they overlap the launch in front)
    int* d_dev = nullptr;              // device words: [0] done_value of the last folded DQN launch, [1] workgroups of folded solo steps that have left
    int solo_left = 0;                 // what [1] will hold once everything enqueued so far has run
    bool dev_obs_valid = false;
    int bound_P = 0;
};

extern "C" int frl_envpool_create(int kind, int n_envs, int n_threads, uint64_t seed, const double* params, int n_params,
                                  frl_envpool** out) {
    if (!out) return fail(FRL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (frl::env_spec(kind).kind < 0) return fail(FRL_ERR_INVALID, "unknown env kind %d", kind);
    if (n_envs < 1 || n_threads < 1 || n_threads > 256) return fail(FRL_ERR_INVALID, "bad n_envs / n_threads");
    frl_envpool* p = new frl_envpool();
    p->pool = new frl::EnvPool(kind, n_envs, n_threads, seed, params, n_params);
    p->host_rng.seed(seed ^ 0xA5A5A5A55A5A5A5Aull);
    *out = p;
    return FRL_OK;
}

extern "C" int frl_envpool_create_callback(int n_envs, int obs_dim, int act_dim, int n_actions, float max_action, frl_env_step_fn step,
                                           frl_env_reset_fn reset, void* user, frl_envpool** out) {
    if (!out) return fail(FRL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_envs < 1 || obs_dim < 1 || act_dim < 1 || n_actions < 0 || !step || !reset) return fail(FRL_ERR_INVALID, "bad callback pool description");
    if (n_actions > 0 && act_dim != 1) return fail(FRL_ERR_INVALID, "discrete envs take one action index (act_dim 1)");
    frl_envpool* p = new frl_envpool();
    p->pool = new frl::EnvPool(n_envs, obs_dim, act_dim, n_actions, max_action, step, reset, user);
    p->host_rng.seed(0xC0FFEEull);
    *out = p;
    return FRL_OK;
}

static void envpool_free_buffers(frl_envpool* p) {
    p->mem.release_all();
    if (p->stream2) hipStreamDestroy(p->stream2);
    p->stream2 = nullptr;
    p->pinned = false;
}

extern "C" int frl_envpool_destroy(frl_envpool* p) {
    if (!p) return FRL_OK;
    envpool_free_buffers(p);
    delete p->pool;
    delete p;
    return FRL_OK;
}

extern "C" int frl_envpool_dims(const frl_envpool* p, int* n_envs, int* obs_dim, int* act_dim, int* n_actions,
                                float* max_action, int* max_steps) {
    if (!p) return fail(FRL_ERR_INVALID, "pool is NULL");
    const frl::EnvSpec& s = p->pool->spec;
    if (n_envs) *n_envs = p->pool->n;
    if (obs_dim) *obs_dim = s.obs_dim;
    if (act_dim) *act_dim = s.act_dim;
    if (n_actions) *n_actions = s.discrete ? s.n_actions : 0;
    if (max_action) *max_action = s.max_action;
    if (max_steps) *max_steps = s.max_steps;
    return FRL_OK;
}

extern "C" int frl_envpool_reset(frl_envpool* p, float* obs_out) {
    if (!p || !obs_out) return fail(FRL_ERR_INVALID, "NULL argument");
    p->pool->reset_all(obs_out);
    if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env reset callback failed (%d)", p->pool->cb_error);
    if (p->pinned) std::memcpy(p->obs, obs_out, sizeof(float) * (size_t)p->pool->n * p->pool->spec.obs_dim);
    p->started = p->pinned;
    p->dev_obs_valid = false;
    return FRL_OK;
}

extern "C" int frl_envpool_set_state(frl_envpool* p, int env, const double* state) {
    if (!p || !state || env < 0 || env >= p->pool->n) return fail(FRL_ERR_INVALID, "bad argument");
    if (p->pool->spec.kind == frl::ENV_CALLBACK) return fail(FRL_ERR_STATE, "a callback pool's envs keep their own state: set it on the env objects");
    std::memcpy(&p->pool->state[(size_t)env * p->pool->spec.state_dim], state, sizeof(double) * p->pool->spec.state_dim);
    p->pool->t[env] = 0;
    p->pool->ep_return[env] = 0.0;
    return FRL_OK;
}

extern "C" int frl_envpool_step(frl_envpool* p, const float* actions, float* next_obs, float* reward, uint8_t* terminated,
                                uint8_t* truncated, float* obs_next) {
    if (!p || !actions || !next_obs || !reward || !terminated || !truncated || !obs_next) return fail(FRL_ERR_INVALID, "NULL argument");
    p->pool->step(actions, next_obs, reward, terminated, truncated, obs_next);
    if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env step callback failed (%d)", p->pool->cb_error);
    return FRL_OK;
}

static int envpool_alloc(frl_engine* e, frl_envpool* p, int a_out) {
    const size_t n = p->pool->n, O = p->pool->spec.obs_dim,
                 A = std::max(std::max(p->pool->spec.act_dim, a_out), p->pool->spec.discrete ? p->pool->spec.n_actions : 1);
    HIP_TRY(p->mem.alloc(&p->obs, n * O, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->next_obs, n * O, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->obs_next, n * O, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->act_out, n * A, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->eps, n * A, MEM_PINNED));
    // env_act, blk and done_flag are also read / written by kernels in place (the folded DQN step): fine-grained coherent whatever
    // HIP_HOST_COHERENT says
    HIP_TRY(p->mem.alloc(&p->env_act, n * A, MEM_PINNED, hipHostMallocCoherent | hipHostMallocMapped));
    HIP_TRY(p->mem.alloc(&p->reward, n, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->term, n, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->trunc, n, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->d_obs, n * O, MEM_DEVICE));
    HIP_TRY(p->mem.alloc(&p->d_out, n * A, MEM_DEVICE));
    HIP_TRY(p->mem.alloc(&p->d_eps, n * A, MEM_DEVICE));
    HIP_TRY(p->mem.alloc(&p->logp, n * A, MEM_PINNED));
    HIP_TRY(p->mem.alloc(&p->d_logp, n * A, MEM_DEVICE));
    // the one block a vector step uploads, sections 16-byte aligned
    const size_t P = e->h.P;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    p->off_row = up16(P * sizeof(float));
    p->off_nobs = up16(p->off_row + n * sizeof(int));
    p->off_onext = up16(p->off_nobs + n * O * sizeof(float));
    p->off_rew = up16(p->off_onext + n * O * sizeof(float));
    p->off_flags = up16(p->off_rew + n * sizeof(float));
    p->blk_bytes = up16(p->off_flags + n);
    HIP_TRY(p->mem.alloc(&p->blk, p->blk_bytes, MEM_PINNED, hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(p->blk, 0, p->blk_bytes);
    HIP_TRY(p->mem.alloc_zero(&p->d_blk, p->blk_bytes, e->stream));
    HIP_TRY(p->mem.alloc(&p->done_flag, 64 / sizeof(int), MEM_PINNED, hipHostMallocCoherent | hipHostMallocMapped));
    *p->done_flag = 0;
    HIP_TRY(p->mem.alloc(&p->go_flag, 64 / sizeof(int), MEM_PINNED, hipHostMallocCoherent | hipHostMallocMapped));
    *p->go_flag = 0;
    HIP_TRY(hipStreamCreateWithFlags(&p->stream2, hipStreamNonBlocking));
    HIP_TRY(p->mem.alloc(&p->d_dev, 64 / sizeof(int), MEM_DEVICE));
    HIP_TRY(p->mem.alloc(&p->d_obs_cur, n * O, MEM_DEVICE));
    HIP_TRY(p->mem.alloc(&p->d_store, n * A, MEM_DEVICE));
    HIP_TRY(p->mem.alloc(&p->d_env, n * A, MEM_DEVICE));
    HIP_TRY(p->mem.alloc_zero(&p->d_ou, n * A, e->stream));
    p->bound_P = (int)P;
    return FRL_OK;
}

// The pool's staging on the engine's device, allocated by the first rollout; a bind that fails half-way leaves nothing behind
static int envpool_bind(frl_engine* e, frl_envpool* p, int a_out) {
    if (p->pinned) return FRL_OK;
    const int rc = envpool_alloc(e, p, a_out);
    if (rc) envpool_free_buffers(p);
    p->pinned = rc == FRL_OK;
    return rc;
}

// One vector step's upload + commit on the device path: the host has filled the block (scale, rows, env outputs, flags).
// blk_dev: the pinned block's device-visible address when the commit launch is to read it in place (small vector steps),
// nullptr: upload it first
static int rollout_commit(frl_engine* e, frl_envpool* p, int E, int aout, const float* logp_dev, int n_logp, const unsigned char* blk_dev = nullptr) {
    const int n = p->pool->n, O = p->pool->spec.obs_dim;
    if (!blk_dev) HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->blk_bytes, hipMemcpyHostToDevice, e->stream));
    const unsigned char* bb = blk_dev ? blk_dev : p->d_blk;
    CommitArgs c;
    memset(&c, 0, sizeof c);
    c.obs_cur = p->d_obs_cur; c.store_act = p->d_store; c.logp = logp_dev;
    c.row = (const int*)(bb + p->off_row);
    c.next_obs = (const float*)(bb + p->off_nobs);
    c.obs_next = (const float*)(bb + p->off_onext);
    c.reward = (const float*)(bb + p->off_rew);
    c.flags = bb + p->off_flags;
    c.n = n; c.E = E; c.O = O; c.aout = aout; c.n_logp = n_logp;
    hipLaunchKernelGGL(replay_commit_kernel, dim3((n * 16 + 255) / 256), dim3(256), 0, e->stream, e->h.replay, e->h.rec, e->h.capacity, c);
    HIP_TRY(hipGetLastError());
    return FRL_OK;      // the block's flags stay in place for the next act launch (OU reset), which precedes the next upload
}

// a learner's exploration multiplier from ITS finished episodes (TD3.py:425-427, SAC.py:548-556)
static float decayed_scale(const frl_rollout_args* ra, const frl::EnvPool* pool, int learner, int E) {
    if (ra->max_episodes <= 0) return 1.f;
    long long eps = 0;
    for (int j = 0; j < E; ++j) eps += pool->ep_count[(size_t)learner * E + j];
    const double remaining = (double)std::max<long long>(0, ra->max_episodes - eps) / (double)ra->max_episodes;
    return (float)(ra->gauss_final_scale + (ra->gauss_init_scale - ra->gauss_final_scale) * remaining);
}

// The rollout-and-update loop for a population, mirroring the reference loop's per-step order (select_action,
// exploration, env.step, add, learn; DQN.py:294-339, TD3.py:403-450, SAC.py:519-566) for P learners x E env instances
// at once.  Per vector step (host_explore = 0):
//   act launch on the device-resident observations, exploration included (Philox)  -D2H env actions->
//   env workers step  -H2D one block: next_obs, obs_next, reward, flags, ring rows, per-learner noise scale->
//   commit launch (records assembled from device-resident obs / actions + the block)  ->  frl_learn (device sampling)
// host_explore = 1 is round 1's loop: obs H2D, action D2H, exploration by a host generator, records staged from the host.
extern "C" int frl_rollout(frl_engine* e, frl_envpool* p, const frl_rollout_args* ra, frl_rollout_stats* out) {
    ENG(e);
    const AlgoTraits& T = algo_traits(e->h.algo);
    if (*T.act_hint) return wrong_engine(e->h, "frl_rollout");      // (no fused collection where the explore launch does not serve; said before the arguments are looked at, as ever)
    if (!p || !ra) return fail(FRL_ERR_INVALID, "NULL argument");
    const EngineDesc& h = e->h;
    const frl::EnvSpec& es = p->pool->spec;
    const int E = ra->envs_per_learner, n = p->pool->n;
    if (!T.rollout) return wrong_engine(h, "frl_rollout");
    if (E < 1 || n != h.P * E) return fail(FRL_ERR_INVALID, "pool has %d envs, engine needs P*E = %d*%d", n, h.P, E);
    if (E > h.capacity) return fail(FRL_ERR_INVALID, "a vector step adds E = %d rows to a ring of %d", E, h.capacity);
    if (es.obs_dim != h.rec.obs_dim[0]) return fail(FRL_ERR_INVALID, "obs_dim mismatch (%d vs %d)", es.obs_dim, h.rec.obs_dim[0]);
    const bool dqn = h.algo == ALGO_DQN, sac = h.algo == ALGO_SAC;
    if (dqn != (es.discrete != 0)) return fail(FRL_ERR_INVALID, "DQN needs a discrete env and the others a continuous one");
    const int A = es.act_dim, O = es.obs_dim;
    if (!dqn && A != h.rec.act_dim[0]) return fail(FRL_ERR_INVALID, "act_dim mismatch");
    if (dqn && es.n_actions != h.n_discrete) return fail(FRL_ERR_INVALID, "n_actions mismatch");
    if (ra->learn.idx || ra->learn.noise) return fail(FRL_ERR_INVALID, "rollout draws on the device: learn.idx/noise must be NULL");
    // a PER engine's priorities move with every sample: the loop of DQN_with_tricks.py (sample -> learn -> update_priorities)
    if (e->per_on && ra->learn_every > 0 && !ra->learn.per)
        return fail(FRL_ERR_STATE, "PER engine: set learn.per (1 reference weighting, 2 per-sample) so the rollout samples and updates priorities");
    if (!e->per_on && ra->learn.per) return fail(FRL_ERR_STATE, "learn.per needs frl_per_enable");
    int kind = ra->explore_kind;
    // 0 = what a memset-zero caller passes: the reference loop's own rule, never a silent "no exploration"
    if (kind <= 0) kind = dqn ? FRL_EXPLORE_EPS_GREEDY : (sac ? FRL_EXPLORE_NONE : FRL_EXPLORE_GAUSS);
    else if (kind == FRL_EXPLORE_OFF) kind = FRL_EXPLORE_NONE;
    else if (kind > FRL_EXPLORE_OU) return fail(FRL_ERR_INVALID, "unknown exploration kind %d", kind);
    if (dqn != (kind == FRL_EXPLORE_EPS_GREEDY)) return fail(FRL_ERR_INVALID, "epsilon-greedy is the discrete rule, Gaussian / OU / none the continuous ones");
    if (ra->host_explore && kind == FRL_EXPLORE_OU) return fail(FRL_ERR_INVALID, "OU exploration runs on the device path only");
    int rc = envpool_bind(e, p, dqn ? 1 : A);
    if (rc) return rc;
    if (p->bound_P != h.P) return fail(FRL_ERR_STATE, "pool was bound to an engine with %d learners", p->bound_P);
    if (!p->started) {
        p->pool->reset_all(p->obs);
        if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env reset callback failed (%d)", p->pool->cb_error);
        p->started = true; p->dev_obs_valid = false;
    }
    const int mode = dqn ? FRL_ACT_ARGMAX : (sac ? FRL_ACT_SAC_SAMPLE : FRL_ACT_TANHHEAD);
    const int aout = dqn ? 1 : A;
    const float ma = dqn ? 1.f : es.max_action;
    const bool dev = !ra->host_explore, host_commit = !dev || e->per_on;     // PER: priorities enter through the staged add path
    std::vector<float> rec(h.rec.width, 0.f);
    long long updates = 0;
    const long long ep0 = p->pool->episodes.load();
    double ret0;
    { std::lock_guard<std::mutex> lk(p->pool->stat_mu); ret0 = p->pool->return_sum; }
    rc = flush_stage(e);
    if (rc) return rc;
    if (dev && !p->dev_obs_valid) {
        HIP_TRY(hipMemcpyAsync(p->d_obs_cur, p->obs, (size_t)n * O * sizeof(float), hipMemcpyHostToDevice, e->stream));
        p->dev_obs_valid = true;
    }
    float* b_scale = (float*)p->blk;
    if (dev) {         // the first act launch of this call reads the multipliers and the episode-end flags before any block went up
        if (ra->max_episodes > 0)
            for (int q = 0; q < h.P; ++q) b_scale[q] = decayed_scale(ra, p->pool, q, E);
        HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->blk_bytes, hipMemcpyHostToDevice, e->stream));     // (the host block always holds the last step's)
    }
    int* b_row = (int*)(p->blk + p->off_row);
    float* b_nobs = (float*)(p->blk + p->off_nobs);
    float* b_onext = (float*)(p->blk + p->off_onext);
    float* b_rew = (float*)(p->blk + p->off_rew);
    unsigned char* b_flags = p->blk + p->off_flags;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const auto t0 = std::chrono::steady_clock::now();
    // FRL_ROLLOUT_TIMING=1: host wall time of the loop's sections on stderr (act + action readback incl. the wait for the
    // previous learn, env step, block fill + commit launches, learn launches)
    const bool timing = env_set("FRL_ROLLOUT_TIMING");
    double t_sec[4] = {0, 0, 0, 0};
    auto tick = std::chrono::steady_clock::now();
    auto lap = [&](int k) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        t_sec[k] += std::chrono::duration<double>(now - tick).count();
        tick = now;
    };
    // DQN on the one-launch update (kernels_dqn2.hip): add(), learn() and the next step's select_action + epsilon-greedy are
    // ONE launch per vector step (FRL_DQN_STEP_FUSE=0: the separate commit / learn / act launches, same draws)
    const bool can_fuse = env_flag("FRL_DQN_STEP_FUSE", true) && dev && !host_commit && dqn && learn_family(e, ra->learn.batch) == FAM_DQN_FUSED;
    // DDPG / TD3 / SAC on the single-learner kernels (kernels_solo.hip): the same fold — add() at the head of the critic launch, the
    // next select_action + exploration at the tail of the step's last launch (FRL_SOLO_STEP_FUSE=0: the separate launches, same draws)
    const bool can_fuse_solo = env_flag("FRL_SOLO_STEP_FUSE", true) && dev && !host_commit && !dqn && learn_family(e, ra->learn.batch) == FAM_SOLO && E <= 1024;
    bool have_action = false;                   // the previous step's launch already produced this step's actions
    // small vector steps: the launch reads the pinned block and writes the env actions in host memory directly (hipHostMalloc
    // memory is device-visible and coherent at kernel boundaries) — a hipMemcpyAsync each way costs more than the launch itself
    // (measured at one env: 58 us from enqueue to the actions on the host for a 28 us launch).  FRL_ROLLOUT_ZEROCOPY=0/1 overrides.
    const bool zero_copy = dev && !host_commit && env_flag("FRL_ROLLOUT_ZEROCOPY", p->blk_bytes <= 64 * 1024);
    unsigned char* blk_dev = nullptr;
    float* env_act_dev = nullptr;
    int* flag_dev = nullptr;
    int* go_dev = nullptr;
    if (zero_copy) {
        HIP_TRY(hipHostGetDevicePointer((void**)&go_dev, p->go_flag, 0));
        HIP_TRY(hipHostGetDevicePointer((void**)&blk_dev, p->blk, 0));
        HIP_TRY(hipHostGetDevicePointer((void**)&env_act_dev, p->env_act, 0));
        HIP_TRY(hipHostGetDevicePointer((void**)&flag_dev, p->done_flag, 0));
    }
    // ... and the host picks the actions up as soon as the launch has flagged them (a release store to a pinned word after
    // the action stores) instead of waiting for the launch to retire and the runtime to notice.  FRL_ROLLOUT_POLL=0: stream sync.
    const bool poll = zero_copy && (can_fuse || can_fuse_solo) && env_flag("FRL_ROLLOUT_POLL", true);
    bool action_on_host = false, action_flagged = false;
    int expect_done = 0;                        // the flag value of the launch whose actions the next step waits for
    // PRE-ARMED launches (small populations on the folded step with the flagged hand-over): the launch of step t + 1 is enqueued as
    // soon as step t's doorbell is rung, on the OTHER of two streams — its arguments are all predictable (ring sizes grow by E per
    // step, Philox counters by two).  It starts while step t's launch runs, draws its rows, waits on a device word for step t's
    // launches to have left, stages its nets and spins on a doorbell word; the host, back from env.step with the block filled, only
    // writes that word.  Launch latency, the gap between two launches of one stream, the index draw and the weight staging then run
    // under step t and the host's turn (kernels.h: DqnStepArgs::go_flag).  FRL_ROLLOUT_PREARM=0/1 overrides.
    const bool prearm_forced = env_flag("FRL_ROLLOUT_PREARM", false), prearm_allowed = env_flag("FRL_ROLLOUT_PREARM", true);
    // (a solo engine's launches need every workgroup resident — the flag hand-overs spin — so an armed launch must fit NEXT to the running
    // one whatever the switch says: 2 x 16 workgroups per learner on the device's CUs (frl_engine::n_cus); past that the armed workgroups would hold the CUs the
    // running step's actor launch is waiting for, until their 2 s bound)
    const bool prearm_fits = can_fuse || (long long)h.P * 2 * std::max(h.solo, 1) <= e->n_cus;
    // (defaults from tools/prearm_soak.py, us per vector step armed / plain: DQN with 8 / 16 / 32 learners 23.8 / 33.1, 27.3 / 34.4, 33.6 / 36.3;
    // TD3 on the solo kernels with 4 / 8 learners 80.9 / 78.4, 100.6 / 89.2 — their armed workgroups' polling costs more than it hides)
    const bool prearm_ok = ((can_fuse && h.P <= 32) || (can_fuse_solo && h.P <= 2) || prearm_forced) && (can_fuse || can_fuse_solo) && prearm_fits && poll && go_dev &&
                           !e->profile && prearm_allowed;
    bool prearmed = false, prearmed_act = false;
    int prearmed_done = 0;
    bool on_alt = false;                        // the last folded launch went to stream2 (the next pre-armed one takes the other stream)
    bool alt_busy = false;                      // stream2 has work that nothing has waited for yet
    // (what arming a launch advanced, to be put back when the launch is cancelled: by ring_or_cancel below, or by the guard on an error return)
    struct ArmSnap {
        unsigned long long rng = 0, pver = 0; unsigned bar = 0; long long total_it = 0; int done_seq = 0, go_seq = 0, solo_left = 0; bool on_alt = false;
        std::chrono::steady_clock::time_point t;
    } snap;
    struct PrearmGuard {                        // an error return with a launch still waiting: tell it to give up; nothing of this call outlives it
        frl_engine* e; decltype(p) pool; const ArmSnap* snap; bool* armed; bool* busy;
        ~PrearmGuard() {
            if (*armed) {
                // the cancel branch of ring_or_cancel: -1 in the doorbell, BOTH streams drained (the armed launch may sit on either), and every
                // counter the arming advanced put back — after a recovered env exception the engine's Philox counters and TD3's policy-delay
                // phase are where a plain step would have left them
                std::atomic_thread_fence(std::memory_order_release);
                *(volatile int*)pool->go_flag = -1;
                hipStreamSynchronize(pool->stream2);
                hipStreamSynchronize(e->stream);
                e->rng_counter = snap->rng; e->param_version = snap->pver; e->solo_bar_base = snap->bar; pool->total_it = snap->total_it;
                pool->done_seq = snap->done_seq; pool->go_seq = snap->go_seq; pool->solo_left = snap->solo_left;
                *(volatile int*)pool->go_flag = 0;
            } else if (*busy) {
                hipStreamSynchronize(pool->stream2);
            }
        }
    } prearm_guard{e, p, &snap, &prearmed, &alt_busy};
    auto join_alt = [&]() -> int {              // work for the engine's stream that is not part of the doorbell protocol: stream2 drained first
        if (alt_busy) { HIP_TRY(hipStreamSynchronize(p->stream2)); alt_busy = false; }
        on_alt = false;
        return FRL_OK;
    };
    if (prearm_ok) {
        const int init[2] = {p->done_seq, 0};
        p->solo_left = 0;
        HIP_TRY(hipMemcpy(p->d_dev, init, sizeof init, hipMemcpyHostToDevice));
        *(volatile int*)p->go_flag = 0;         // (an earlier call that gave a launch up left -1 here)
    }
    // A pre-armed launch gives up after 2 s of spinning (a bound on what a stuck host can do to the GPU).  An env whose step takes that
    // long must not lose its update to that: past kArmPatience between arming and the doorbell the host CANCELS the launch for certain
    // (-1 in the doorbell, both streams drained — a launch that gives up has touched nothing), puts every counter the arming advanced
    // back, and the caller launches the step the plain way with the same arguments.  FRL_ROLLOUT_ARM_PATIENCE_MS: the bound in
    // milliseconds (tests: 0 = every armed launch is cancelled and replayed).
    const char* apf = getenv("FRL_ROLLOUT_ARM_PATIENCE_MS");
    const double arm_patience = apf ? atof(apf) * 1e-3 : 1.0;
    auto arm_snapshot = [&]() {
        snap.rng = e->rng_counter; snap.pver = e->param_version; snap.bar = e->solo_bar_base; snap.total_it = p->total_it;
        snap.done_seq = p->done_seq; snap.go_seq = p->go_seq; snap.solo_left = p->solo_left; snap.on_alt = on_alt;
        snap.t = std::chrono::steady_clock::now();
    };
    // 1: the doorbell is rung; 0: the launch was cancelled, the caller launches this step itself; < 0: error
    auto ring_or_cancel = [&]() -> int {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - snap.t).count() >= arm_patience) {
            std::atomic_thread_fence(std::memory_order_release);
            *(volatile int*)p->go_flag = -1;
            hipError_t he = hipStreamSynchronize(p->stream2);
            if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
            if (he != hipSuccess) return -fail(FRL_ERR_HIP, "cancelling a pre-armed launch: %s", hipGetErrorString(he));
            alt_busy = false;
            e->rng_counter = snap.rng; e->param_version = snap.pver; e->solo_bar_base = snap.bar; p->total_it = snap.total_it;
            p->done_seq = snap.done_seq; p->go_seq = snap.go_seq; p->solo_left = snap.solo_left; on_alt = snap.on_alt;
            *(volatile int*)p->go_flag = 0;
            prearmed = false;
            return 0;
        }
        std::atomic_thread_fence(std::memory_order_release);
        *(volatile int*)p->go_flag = p->go_seq;
        prearmed = false;
        have_action = prearmed_act; action_on_host = true; action_flagged = prearmed_act; expect_done = prearmed_done;
        return 1;
    };
    for (int step = 0; step < ra->n_steps; ++step) {
        float* nobs = dev ? b_nobs : p->next_obs;
        float* onext = dev ? b_onext : p->obs_next;
        float* rew = dev ? b_rew : p->reward;
        if (dev && have_action) {
            if (!action_on_host) HIP_TRY(hipMemcpyAsync(p->env_act, p->d_env, (size_t)n * aout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            bool seen = false;
            if (action_flagged) {               // spin on the pinned word for up to ~2 s, then fall back to the stream
                volatile int* fl = p->done_flag;
                const auto t_spin = std::chrono::steady_clock::now();
                for (long long it = 0; !seen; ++it) {
                    if (*fl == expect_done) { seen = true; break; }
                    if ((it & 0xfff) == 0xfff && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_spin).count() > 2.0) break;
                }
                std::atomic_thread_fence(std::memory_order_acquire);
            }
            if (!seen) {
                if (alt_busy) { HIP_TRY(hipStreamSynchronize(p->stream2)); alt_busy = false; }
                HIP_TRY(hipStreamSynchronize(e->stream));
                { const int rs = solo_err_check(e); if (rs) return rs; }     // (a launch that gave up left no actions: do not step the envs on the old ones)
            }
        } else if (dev) {
            ActExplore ex;
            ex.x.kind = kind; ex.x.epsilon = ra->epsilon; ex.x.sigma = ra->explore_sigma; ex.x.scale = 1.f; ex.x.max_action = ma;
            ex.x.ou_theta = ra->ou_theta; ex.x.ou_sigma = ra->ou_sigma; ex.x.ou_dt = ra->ou_dt;
            const unsigned char* bb = zero_copy ? blk_dev : p->d_blk;      // the last block: in place in pinned memory, or its upload
            ex.scale_dev = ra->max_episodes > 0 ? (const float*)bb : nullptr;
            ex.ou_state_dev = p->d_ou; ex.flags_dev = bb + p->off_flags; ex.env_out_dev = zero_copy ? env_act_dev : p->d_env;
            ex.device_eps = true;
            rc = join_alt();
            if (rc) return rc;
            rc = launch_act(e, 0, mode, 0, 0, E, O, p->d_obs_cur, nullptr, p->d_store, nullptr, &ex);
            if (rc) return rc;
            if (!zero_copy) HIP_TRY(hipMemcpyAsync(p->env_act, p->d_env, (size_t)n * aout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            if (host_commit && !dqn) HIP_TRY(hipMemcpyAsync(p->act_out, p->d_store, (size_t)n * aout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(p->d_obs, p->obs, (size_t)n * O * sizeof(float), hipMemcpyHostToDevice, e->stream));
            if (sac) {
                for (size_t i = 0; i < (size_t)n * A; ++i) p->eps[i] = (float)p->host_rng.normal();
                HIP_TRY(hipMemcpyAsync(p->d_eps, p->eps, (size_t)n * A * sizeof(float), hipMemcpyHostToDevice, e->stream));
            }
            rc = launch_act(e, 0, mode, 0, 0, E, O, p->d_obs, sac ? p->d_eps : nullptr, p->d_out, nullptr);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(p->act_out, p->d_out, (size_t)n * aout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            // exploration (host generator): epsilon-greedy (DQN.py:307-310) / Gaussian action noise (TD3.py:412)
            for (int i = 0; i < n; ++i) {
                if (dqn) {
                    float a = p->act_out[i];
                    if (p->host_rng.uniform() < ra->epsilon) a = (float)(int)(p->host_rng.uniform() * es.n_actions);
                    p->act_out[i] = a;
                    p->env_act[i] = a;
                } else {
                    const float sc = kind == FRL_EXPLORE_GAUSS ? decayed_scale(ra, p->pool, i / E, E) * ra->explore_sigma : 0.f;
                    for (int c = 0; c < A; ++c) {
                        float v = p->act_out[(size_t)i * A + c] * ma;
                        if (sc > 0.f) v += sc * ma * (float)p->host_rng.normal();
                        p->env_act[(size_t)i * A + c] = v < -ma ? -ma : (v > ma ? ma : v);
                    }
                }
            }
        }
        lap(0);
        p->pool->step(p->env_act, nobs, rew, p->term, p->trunc, onext);
        lap(1);
        if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env step callback failed (%d)", p->pool->cb_error);
        if (host_commit) {
            const float* stored = (dev && dqn) ? p->env_act : p->act_out;       // DQN stores the explored index
            for (int i = 0; i < n; ++i) {               // add(obs, action, reward, next_obs, terminated)
                float* r = rec.data();
                std::memcpy(r + h.rec.obs_off[0], p->obs + (size_t)i * O, sizeof(float) * O);
                std::memcpy(r + h.rec.act_off[0], stored + (size_t)i * aout, sizeof(float) * aout);
                r[h.rec.rew_off] = rew[i];
                r[h.rec.done_off] = p->term[i] ? 1.f : 0.f;
                std::memcpy(r + h.rec.nobs_off[0], nobs + (size_t)i * O, sizeof(float) * O);
                rc = stage_one(e, i / E, r);
                if (rc) return rc;
            }
        }
        if (dev) {
            for (int i = 0; i < n; ++i) {
                const int q = i / E;
                b_flags[i] = (unsigned char)((p->term[i] ? 1 : 0) | ((p->term[i] || p->trunc[i]) ? 2 : 0));
                if (!host_commit) {                     // Buffer.add's cursor arithmetic (Buffer.py:36-38), the row written on the device
                    b_row[i] = e->index[q];
                    e->index[q] = (e->index[q] + 1) % h.capacity;
                    if (e->size[q] < h.capacity) e->size[q]++;
                }
            }
            for (int q = 0; q < h.P; ++q) b_scale[q] = decayed_scale(ra, p->pool, q, E);
            int msz = h.capacity;
            for (int q = 0; q < h.P; ++q) msz = std::min(msz, e->size[q]);
            const bool learn_due = ra->learn_every > 0 && (step + 1) % ra->learn_every == 0 && msz > ra->start_steps && msz >= 2 * ra->learn.batch;
            have_action = false;
            if (can_fuse && learn_due) {
                // the step's launch: arguments of vector step `st` (this one, or — pre-armed — the next one)
                auto launch_step = [&](int st, int size_at_launch, bool armed) -> int {
                    const unsigned char* bb = zero_copy ? blk_dev : p->d_blk;
                    DqnStepArgs sa;
                    memset(&sa, 0, sizeof sa);
                    sa.commit = 1; sa.act = (st + 1 < ra->n_steps) ? 1 : 0;
                    sa.E = E; sa.O = O;
                    sa.obs_cur = p->d_obs_cur; sa.store_act = p->d_store;
                    sa.row = (const int*)(bb + p->off_row);
                    sa.next_obs = (const float*)(bb + p->off_nobs);
                    sa.obs_next = (const float*)(bb + p->off_onext);
                    sa.reward = (const float*)(bb + p->off_rew);
                    sa.flags = bb + p->off_flags;
                    sa.act_out = p->d_store; sa.env_out = zero_copy ? env_act_dev : p->d_env;
                    const bool flagged = poll && sa.act;
                    if (armed) { sa.go_flag = go_dev; sa.go_value = ++p->go_seq; sa.dev_wait = p->done_seq; }
                    if (flagged) { sa.done_flag = flag_dev; sa.done_value = ++p->done_seq; if (prearm_ok) sa.dev_done = p->d_dev; }
                    if (armed) { sa.dev_done = p->d_dev; sa.err = e->d_solo_err; }
                    else { const int rj = join_alt(); if (rj) return rj; }
                    hipStream_t lst = armed && !on_alt ? p->stream2 : nullptr;
                    sa.epsilon = ra->epsilon;
                    sa.act_counter = e->rng_counter + 1;    // learn() takes the next counter value, the act draw the one after (as separate launches do)
                    frl_learn_args la = ra->learn;
                    la.stats_out = nullptr;
                    ++p->total_it;
                    const int r2 = learn_impl(e, &la, &sa, nullptr, size_at_launch, lst);
                    if (r2) return r2;
                    if (armed) { on_alt = (lst != nullptr); alt_busy = alt_busy || on_alt; }
                    if (sa.act) e->rng_counter++;
                    if (armed) { prearmed = true; prearmed_act = sa.act != 0; prearmed_done = sa.done_value; }
                    else { have_action = sa.act != 0; action_on_host = zero_copy; action_flagged = flagged; expect_done = sa.done_value; }
                    return FRL_OK;
                };
                int rung = 0;
                if (prearmed) {                 // this step's launch is already there, spinning: the block is complete -> ring the doorbell
                    rung = ring_or_cancel();
                    if (rung < 0) return -rung;
                }
                if (!rung) {
                    if (!zero_copy) HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->blk_bytes, hipMemcpyHostToDevice, e->stream));
                    rc = launch_step(step, -1, false);
                    if (rc) return rc;
                }
                updates += h.P;
                std::memcpy(p->obs, onext, sizeof(float) * (size_t)n * O);
                if (prearm_ok && step + 1 < ra->n_steps) {          // the next step's launch, now: will it be a learn step?
                    int msz1 = h.capacity;
                    for (int q = 0; q < h.P; ++q) msz1 = std::min(msz1, std::min(e->size[q] + E, h.capacity));
                    const bool due1 = ra->learn_every > 0 && (step + 2) % ra->learn_every == 0 && msz1 > ra->start_steps && msz1 >= 2 * ra->learn.batch;
                    if (due1) {
                        arm_snapshot();
                        rc = launch_step(step + 1, msz1, true);
                        if (rc) return rc;
                    }
                }
                lap(2);
                lap(3);
                continue;
            }
            if (can_fuse_solo && learn_due) {
                auto launch_step = [&](int st, int size_at_launch, bool armed) -> int {
                    const unsigned char* bb = zero_copy ? blk_dev : p->d_blk;
                    SoloStepArgs ss;
                    memset(&ss, 0, sizeof ss);
                    ss.act = (st + 1 < ra->n_steps) ? 1 : 0;
                    ss.c.obs_cur = p->d_obs_cur; ss.c.store_act = p->d_store;
                    ss.c.row = (const int*)(bb + p->off_row);
                    ss.c.next_obs = (const float*)(bb + p->off_nobs);
                    ss.c.obs_next = (const float*)(bb + p->off_onext);
                    ss.c.reward = (const float*)(bb + p->off_rew);
                    ss.c.flags = bb + p->off_flags;
                    ss.c.n = n; ss.c.E = E; ss.c.O = O; ss.c.aout = aout;
                    if (ss.act) {
                        ActExplore ex;                          // exactly what the separate act launch of the next step would be given
                        ex.x.kind = kind; ex.x.epsilon = ra->epsilon; ex.x.sigma = ra->explore_sigma; ex.x.scale = 1.f; ex.x.max_action = ma;
                        ex.x.ou_theta = ra->ou_theta; ex.x.ou_sigma = ra->ou_sigma; ex.x.ou_dt = ra->ou_dt;
                        ex.scale_dev = ra->max_episodes > 0 ? (const float*)bb : nullptr;
                        ex.ou_state_dev = p->d_ou; ex.flags_dev = bb + p->off_flags; ex.env_out_dev = zero_copy ? env_act_dev : p->d_env;
                        ex.device_eps = true;
                        const int r1 = launch_act(e, 0, mode, 0, 0, E, O, p->d_obs_cur, nullptr, p->d_store, nullptr, &ex, &ss.act_args);
                        if (r1) return r1;
                        ss.act_args.rng_counter = e->rng_counter + 1;      // learn() takes the next counter value, the act draw the one after (as separate launches do)
                    }
                    ss.ticket = e->d_solo_ticket;
                    ss.bar2 = e->d_solo_bar + (size_t)h.P * kSoloWG;
                    const bool flagged = poll && ss.act;
                    if (flagged) { ss.done_flag = flag_dev; ss.done_value = ++p->done_seq; }
                    if (armed) { ss.go_flag = go_dev; ss.go_value = ++p->go_seq; ss.dev_wait = p->solo_left; }
                    else { const int rj = join_alt(); if (rj) return rj; }
                    if (prearm_ok) ss.dev_cnt = p->d_dev + 1;
                    hipStream_t lst = armed && !on_alt ? p->stream2 : nullptr;
                    frl_learn_args la = ra->learn;
                    la.stats_out = nullptr;
                    ++p->total_it;
                    if (h.algo == ALGO_TD3) la.do_actor = (ra->policy_freq <= 1) || (p->total_it % ra->policy_freq == 0);
                    const int r2 = learn_impl(e, &la, nullptr, &ss, size_at_launch, lst);
                    if (r2) return r2;
                    if (armed) { on_alt = (lst != nullptr); alt_busy = alt_busy || on_alt; }
                    p->solo_left += h.P * h.solo * ((h.algo == ALGO_TD3 && !la.do_actor) ? 1 : 2);
                    if (ss.act) e->rng_counter++;
                    if (armed) { prearmed = true; prearmed_act = ss.act != 0; prearmed_done = ss.done_value; }
                    else { have_action = ss.act != 0; action_on_host = zero_copy; action_flagged = flagged; expect_done = ss.done_value; }
                    return FRL_OK;
                };
                int rung = 0;
                if (prearmed) {
                    rung = ring_or_cancel();
                    if (rung < 0) return -rung;
                }
                if (!rung) {
                    if (!zero_copy) HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->blk_bytes, hipMemcpyHostToDevice, e->stream));
                    have_action = false;
                    rc = launch_step(step, -1, false);
                    if (rc) return rc;
                }
                updates += h.P;
                std::memcpy(p->obs, onext, sizeof(float) * (size_t)n * O);
                if (prearm_ok && step + 1 < ra->n_steps) {
                    int msz1 = h.capacity;
                    for (int q = 0; q < h.P; ++q) msz1 = std::min(msz1, std::min(e->size[q] + E, h.capacity));
                    const bool due1 = ra->learn_every > 0 && (step + 2) % ra->learn_every == 0 && msz1 > ra->start_steps && msz1 >= 2 * ra->learn.batch;
                    if (due1) {
                        arm_snapshot();
                        rc = launch_step(step + 1, msz1, true);
                        if (rc) return rc;
                    }
                }
                lap(2);
                lap(3);
                continue;
            }
            rc = join_alt();
            if (rc) return rc;
            if (host_commit) {                          // the records went through the stage; the device still needs obs_next and the flags
                HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->blk_bytes, hipMemcpyHostToDevice, e->stream));
                HIP_TRY(hipMemcpyAsync(p->d_obs_cur, p->d_blk + p->off_onext, (size_t)n * O * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
            } else {
                rc = rollout_commit(e, p, E, aout, nullptr, 0, zero_copy ? blk_dev : nullptr);
                if (rc) return rc;
            }
            std::memcpy(p->obs, onext, sizeof(float) * (size_t)n * O);          // host mirror of what the policy sees next
        } else {
            std::swap(p->obs, p->obs_next);
            p->dev_obs_valid = false;
        }
        int min_size = h.capacity;
        for (int q = 0; q < h.P; ++q) min_size = std::min(min_size, e->size[q]);
        lap(2);
        if (ra->learn_every > 0 && (step + 1) % ra->learn_every == 0 && min_size > ra->start_steps &&
            min_size >= 2 * ra->learn.batch) {
            frl_learn_args la = ra->learn;
            la.stats_out = nullptr;
            ++p->total_it;
            if (h.algo == ALGO_TD3) la.do_actor = (ra->policy_freq <= 1) || (p->total_it % ra->policy_freq == 0);
            if (la.per) { rc = frl_per_sample(e, la.batch, nullptr, nullptr, nullptr); if (rc) return rc; }
            rc = frl_learn(e, &la);
            if (rc) return rc;
            if (la.per) { rc = frl_per_update(e, la.batch, nullptr, nullptr); if (rc) return rc; }
            updates += h.P;
        }
        lap(3);
    }
    rc = join_alt();
    if (rc) return rc;
    rc = flush_stage(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = solo_err_check(e);
    if (rc) return rc;
    if (timing && ra->n_steps > 0)
        fprintf(stderr, "frl_rollout: per vector step  act + readback (waits for the learn) %.1f us, env step %.1f us, block + commit %.1f us, learn launches %.1f us\n",
                t_sec[0] / ra->n_steps * 1e6, t_sec[1] / ra->n_steps * 1e6, t_sec[2] / ra->n_steps * 1e6, t_sec[3] / ra->n_steps * 1e6);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out) {
        out->env_steps = (long long)ra->n_steps * n;
        out->updates = updates;
        out->episodes = p->pool->episodes.load() - ep0;
        { std::lock_guard<std::mutex> lk(p->pool->stat_mu); out->return_sum = p->pool->return_sum - ret0; }
        out->seconds = secs;
    }
    return FRL_OK;
}

// On-policy collector + learn for a population of PPO learners (BASELINE config 3: PPO with vectorised envs).  The
// reference steps ONE env for `horizon` steps and then calls learn() (PPO_with_tricks.py:524-569); here every learner
// steps E env instances for horizon / E vector steps.  Env j's transitions occupy the contiguous ring rows
// [j*Tseg, (j+1)*Tseg) in time order, and the last row of every segment carries adv_done = 1, so the GAE scan over the
// ring restarts there exactly as it restarts at the end of the reference's single-env horizon: the row still
// bootstraps from V(next_obs) (done = terminated only), nothing flows in from the following segment (:308-311).
extern "C" int frl_ppo_rollout(frl_engine* e, frl_envpool* p, const frl_ppo_rollout_args* ra, frl_rollout_stats* out) {
    ENG(e);
    if (!p || !ra) return fail(FRL_ERR_INVALID, "NULL argument");
    const EngineDesc& h = e->h;
    const frl::EnvSpec& es = p->pool->spec;
    if (h.algo != ALGO_PPO) return wrong_engine(h, "frl_ppo_rollout");
    if (h.beta_actor) return fail(FRL_ERR_STATE, "frl_ppo_rollout: Gaussian and Categorical actors only");
    const int E = ra->envs_per_learner, Tseg = ra->steps_per_env, n = p->pool->n, T = E * Tseg;
    if (E < 1 || Tseg < 1 || n != h.P * E) return fail(FRL_ERR_INVALID, "pool has %d envs, engine needs P*E = %d*%d", n, h.P, E);
    if (T != ra->learn.horizon || T > h.capacity) return fail(FRL_ERR_INVALID, "horizon %d != E*steps_per_env = %d (capacity %d)", ra->learn.horizon, T, h.capacity);
    if (ra->learn.perms || ra->learn.loss_trace_out || ra->learn.adv_out || ra->learn.vtarget_out || ra->learn.gae_mode)
        return fail(FRL_ERR_INVALID, "rollout learns with device-drawn permutations: perms / outputs must be NULL, gae_mode 0");
    const bool disc = h.n_discrete > 0;
    if (disc != (es.discrete != 0)) return fail(FRL_ERR_INVALID, "discrete policy needs a discrete env and vice versa");
    const int A = es.act_dim, O = es.obs_dim, nA = es.n_actions;
    if (O != h.rec.obs_dim[0]) return fail(FRL_ERR_INVALID, "obs_dim mismatch (%d vs %d)", O, h.rec.obs_dim[0]);
    if (!disc && A != h.rec.act_dim[0]) return fail(FRL_ERR_INVALID, "act_dim mismatch");
    if (disc && nA != h.n_discrete) return fail(FRL_ERR_INVALID, "n_actions mismatch");
    const int stored = disc ? 1 : A;                   // Buffer act_dim = log-prob columns (PPO_file/Buffer.py:3-9)
    if (h.rec.extra != stored + 1) return fail(FRL_ERR_STATE, "ring needs extra_cols = %d (log-probs + adv_done)", stored + 1);
    int rc = envpool_bind(e, p, stored);
    if (rc) return rc;
    if (p->bound_P != h.P) return fail(FRL_ERR_STATE, "pool was bound to an engine with %d learners", p->bound_P);
    if (!p->started) {
        p->pool->reset_all(p->obs);
        if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env reset callback failed (%d)", p->pool->cb_error);
        p->started = true; p->dev_obs_valid = false;
    }
    const int mode = disc ? FRL_ACT_CAT_SAMPLE : FRL_ACT_PPO_SAMPLE;
    const float ma = disc ? 1.f : es.max_action;
    const int n_mb = (T + ra->learn.minibatch - 1) / ra->learn.minibatch;
    long long updates = 0;
    const long long ep0 = p->pool->episodes.load();
    double ret0;
    { std::lock_guard<std::mutex> lk(p->pool->stat_mu); ret0 = p->pool->return_sum; }
    rc = flush_stage(e);
    if (rc) return rc;
    if (!p->dev_obs_valid) {
        HIP_TRY(hipMemcpyAsync(p->d_obs_cur, p->obs, (size_t)n * O * sizeof(float), hipMemcpyHostToDevice, e->stream));
        p->dev_obs_valid = true;
    }
    int* b_row = (int*)(p->blk + p->off_row);
    float* b_nobs = (float*)(p->blk + p->off_nobs);
    float* b_onext = (float*)(p->blk + p->off_onext);
    float* b_rew = (float*)(p->blk + p->off_rew);
    unsigned char* b_flags = p->blk + p->off_flags;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < ra->n_iters; ++it) {
        for (int t = 0; t < Tseg; ++t) {
            // Normal.sample(): mean + std * N(0,1) (:240-242); Categorical.sample(): argmax(p / q), q ~ Exp(1) (:249-251) — the
            // variates come from the launch's Philox stream; action_ = clip(action * max_action) (:529-530) in the same launch
            ActExplore ex;
            ex.x.kind = FRL_EXPLORE_NONE; ex.x.max_action = ma; ex.x.scale = 1.f;
            ex.env_out_dev = p->d_env; ex.device_eps = true;
            rc = launch_act(e, 0, mode, 0, 0, E, O, p->d_obs_cur, nullptr, p->d_store, p->d_logp, &ex);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(p->env_act, p->d_env, (size_t)n * stored * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            p->pool->step(p->env_act, b_nobs, b_rew, p->term, p->trunc, b_onext);
            if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env step callback failed (%d)", p->pool->cb_error);
            for (int i = 0; i < n; ++i) {     // add(obs, action, reward, next_obs, terminated, log_pi, done): flags + the ring row
                const bool ended = p->term[i] || p->trunc[i];
                b_flags[i] = (unsigned char)((p->term[i] ? 1 : 0) | (ended ? 2 : 0) | ((ended || t == Tseg - 1) ? 4 : 0));
                b_row[i] = (i % E) * Tseg + t;                       // env j's segment is contiguous in the ring
            }
            rc = rollout_commit(e, p, E, stored, p->d_logp, stored);
            if (rc) return rc;
        }
        std::memcpy(p->obs, b_onext, sizeof(float) * (size_t)n * O);
        for (int q = 0; q < h.P; ++q) { e->index[q] = T % h.capacity; e->size[q] = T; }
        rc = frl_ppo_learn(e, &ra->learn);
        if (rc) return rc;
        updates += (long long)h.P * ra->learn.k_epochs * n_mb;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out) {
        out->env_steps = (long long)ra->n_iters * Tseg * n;
        out->updates = updates;
        out->episodes = p->pool->episodes.load() - ep0;
        { std::lock_guard<std::mutex> lk(p->pool->stat_mu); out->return_sum = p->pool->return_sum - ret0; }
        out->seconds = secs;
    }
    return FRL_OK;
}
