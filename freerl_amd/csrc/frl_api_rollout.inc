// Env pool + rollout collector entry points (included at the end of frl_api.hip).
#include "envpool.hpp"
#include "rollout_plan.hpp"
#define FRL_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

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
    frl::BlkLayout lay;                // its sections (rollout_plan.hpp)
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
    p->lay = BlkLayout(e->h.P, n, O);          // the one block a vector step uploads, sections 16-byte aligned (rollout_plan.hpp)
    HIP_TRY(p->mem.alloc(&p->blk, p->lay.bytes, MEM_PINNED, hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(p->blk, 0, p->lay.bytes);
    HIP_TRY(p->mem.alloc_zero(&p->d_blk, p->lay.bytes, e->stream));
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
    p->bound_P = e->h.P;
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

// What both collectors do in front of their loops — the pool bound to this engine, the envs reset once, the counters their statistics are
// differences of, staged rows flushed and (dev) the observations on the device — and behind them: frl_rollout_stats
struct RolloutTally { long long ep0 = 0; double ret0 = 0; std::chrono::steady_clock::time_point t0; };      // t0: set by the collector once its first uploads have landed
static int rollout_begin(frl_engine* e, frl_envpool* p, int a_out, bool dev, RolloutTally* t) {
    FRL_TRY(envpool_bind(e, p, a_out));
    if (p->bound_P != e->h.P) return fail(FRL_ERR_STATE, "pool was bound to an engine with %d learners", p->bound_P);
    if (!p->started) {
        p->pool->reset_all(p->obs);
        if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env reset callback failed (%d)", p->pool->cb_error);
        p->started = true; p->dev_obs_valid = false;
    }
    t->ep0 = p->pool->episodes.load();
    { std::lock_guard<std::mutex> lk(p->pool->stat_mu); t->ret0 = p->pool->return_sum; }
    FRL_TRY(flush_stage(e));
    if (dev && !p->dev_obs_valid) {
        HIP_TRY(hipMemcpyAsync(p->d_obs_cur, p->obs, (size_t)p->pool->n * p->pool->spec.obs_dim * sizeof(float), hipMemcpyHostToDevice, e->stream));
        p->dev_obs_valid = true;
    }
    return FRL_OK;
}
static void rollout_finish(frl_envpool* p, const RolloutTally& t, long long env_steps, long long updates, frl_rollout_stats* out) {
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t.t0).count();
    if (!out) return;
    out->env_steps = env_steps;
    out->updates = updates;
    out->episodes = p->pool->episodes.load() - t.ep0;
    { std::lock_guard<std::mutex> lk(p->pool->stat_mu); out->return_sum = p->pool->return_sum - t.ret0; }
    out->seconds = secs;
}

// the block's sections as a commit reads them (CommitArgs and DqnStepArgs name them alike)
template <class Args> static void set_sections(Args& a, const BlkView& v) {
    a.row = v.row; a.next_obs = v.next_obs; a.obs_next = v.obs_next; a.reward = v.reward; a.flags = v.flags;
}

// One vector step's upload + commit on the device path: the host has filled the block (scale, rows, env outputs, flags).
// blk_dev: the pinned block's device-visible address when the commit launch is to read it in place (small vector steps),
// nullptr: upload it first
static int rollout_commit(frl_engine* e, frl_envpool* p, int E, int aout, const float* logp_dev, int n_logp, unsigned char* blk_dev = nullptr) {
    const int n = p->pool->n, O = p->pool->spec.obs_dim;
    if (!blk_dev) HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->lay.bytes, hipMemcpyHostToDevice, e->stream));
    CommitArgs c;
    memset(&c, 0, sizeof c);
    c.obs_cur = p->d_obs_cur; c.store_act = p->d_store; c.logp = logp_dev;
    set_sections(c, p->lay.view(blk_dev ? blk_dev : p->d_blk));
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

// frl_rollout's knobs (rollout_plan.hpp: RolloutKnobs), read at EVERY call
static RolloutKnobs rollout_knobs() {
    auto tri = [](const char* name) { return env_set(name) ? (int)env_flag(name, false) : -1; };
    RolloutKnobs k;
    k.timing = env_set("FRL_ROLLOUT_TIMING");
    k.dqn_step_fuse = env_flag("FRL_DQN_STEP_FUSE", k.dqn_step_fuse);
    k.solo_step_fuse = env_flag("FRL_SOLO_STEP_FUSE", k.solo_step_fuse);
    k.zero_copy = tri("FRL_ROLLOUT_ZEROCOPY");
    k.poll = env_flag("FRL_ROLLOUT_POLL", k.poll);
    k.prearm = tri("FRL_ROLLOUT_PREARM");
    k.arm_patience_ms = env_double("FRL_ROLLOUT_ARM_PATIENCE_MS", k.arm_patience_ms);
    return k;
}
static RolloutFacts rollout_facts(const frl_engine* e, const frl_envpool* p, int batch) {
    const EngineDesc& h = e->h;
    const frl::EnvSpec& es = p->pool->spec;
    RolloutFacts f;
    f.algo = h.algo; f.P = h.P; f.capacity = h.capacity; f.n_discrete = h.n_discrete; f.rec_obs_dim = h.rec.obs_dim[0]; f.rec_act_dim = h.rec.act_dim[0];
    f.per_on = e->per_on; f.profile = e->profile; f.n_cus = e->n_cus; f.solo = h.solo; f.family = learn_family(e, batch);
    f.n = p->pool->n; f.obs_dim = es.obs_dim; f.act_dim = es.act_dim; f.n_actions = es.n_actions; f.discrete = es.discrete != 0; f.max_action = es.max_action;
    f.blk_bytes = BlkLayout(h.P, f.n, es.obs_dim).bytes;      // (what the pool's block measures once it is bound to this engine)
    return f;
}

// One frl_rollout call past its plan: engine, pool, arguments, the device-visible aliases and the two small pieces of protocol state the
// vector steps hand each other.  frl_rollout below is the sequence of its steps.
struct RolloutRun {
    frl_engine* const e;
    frl_envpool* const p;
    const frl_rollout_args* const ra;
    const RolloutPlan plan;
    const EngineDesc& h;
    const int E, n, O, A;               // envs per learner, envs, obs_dim and act_dim of the pool
    const BlkView host;                 // the pinned block as the host fills it
    BlkView in;                         // ... as the launches read it: its upload, or in place (zero copy) at blk_dev, its device-visible alias
    unsigned char* blk_dev = nullptr;
    float* env_out;                     // where a launch leaves the env actions: d_env, or (zero copy) pinned env_act's alias
    int *flag_dev = nullptr, *go_dev = nullptr;      // done_flag's and go_flag's aliases
    std::vector<float> rec;             // one record of the staged add path
    float *nobs = nullptr, *onext = nullptr, *rew = nullptr;      // where this step's env outputs go
    long long updates = 0;
    // The action hand-over.  have_action: the previous step's launch already produced this step's actions; on_host: in pinned memory (no
    // copy back); flagged: and it says so in done_flag; expect_done: with this value
    struct { bool have_action = false, on_host = false, flagged = false; int expect_done = 0; } act;
    // The arming: a launch enqueued a step ahead (armed, whether it acts and its done value).  on_alt: the last folded launch went to stream2
    // (the next armed one takes the other stream); alt_busy: stream2 has work that nothing has waited for yet.  Behind them what arming
    // advanced and when, to be put back when the launch is cancelled
    struct {
        bool armed = false, armed_act = false, on_alt = false, alt_busy = false;
        int armed_done = 0;
        unsigned long long rng = 0, pver = 0; unsigned bar = 0; long long total_it = 0; int done_seq = 0, go_seq = 0, solo_left = 0; bool was_on_alt = false;
        std::chrono::steady_clock::time_point t;
    } arm;
    // FRL_ROLLOUT_TIMING=1: host wall time of the loop's sections on stderr (act + action readback incl. the wait for the
    // previous learn, env step, block fill + commit launches, learn launches)
    double t_sec[4] = {0, 0, 0, 0};
    std::chrono::steady_clock::time_point tick;

    RolloutRun(frl_engine* e_, frl_envpool* p_, const frl_rollout_args* ra_, const RolloutPlan& pl)
        : e(e_), p(p_), ra(ra_), plan(pl), h(e_->h), E(ra_->envs_per_learner), n(p_->pool->n), O(p_->pool->spec.obs_dim), A(p_->pool->spec.act_dim),
          host(p_->lay.view(p_->blk)), in(p_->lay.view(p_->d_blk)), env_out(p_->d_env), rec(e_->h.rec.width, 0.f) {}
    // an error return with a launch still waiting: tell it to give up; nothing of this call outlives it
    ~RolloutRun() { if (arm.armed) (void)cancel_armed(); else if (arm.alt_busy) (void)hipStreamSynchronize(p->stream2); }
    void lap(int k) {
        if (!plan.timing) return;
        const auto now = std::chrono::steady_clock::now();
        t_sec[k] += std::chrono::duration<double>(now - tick).count();
        tick = now;
    }
    int min_ring_size(int grow = 0) const {      // the smallest ring once every learner has added `grow` more rows
        int m = h.capacity;
        for (int q = 0; q < h.P; ++q) m = std::min(m, std::min(e->size[q] + grow, h.capacity));
        return m;
    }
    // the call's first block, the clock, the aliases and the arming's device words
    int open(RolloutTally* t) {
        if (plan.dev) {         // the first act launch of this call reads the multipliers and the episode-end flags before any block went up
            if (ra->max_episodes > 0)
                for (int q = 0; q < h.P; ++q) host.scale[q] = decayed_scale(ra, p->pool, q, E);
            HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->lay.bytes, hipMemcpyHostToDevice, e->stream));     // (the host block always holds the last step's)
        }
        HIP_TRY(hipStreamSynchronize(e->stream));
        t->t0 = tick = std::chrono::steady_clock::now();
        if (plan.zero_copy) {
            HIP_TRY(hipHostGetDevicePointer((void**)&go_dev, p->go_flag, 0));
            HIP_TRY(hipHostGetDevicePointer((void**)&blk_dev, p->blk, 0));
            HIP_TRY(hipHostGetDevicePointer((void**)&env_out, p->env_act, 0));
            HIP_TRY(hipHostGetDevicePointer((void**)&flag_dev, p->done_flag, 0));
            in = p->lay.view(blk_dev);
        }
        if (plan.prearm) {
            const int init[2] = {p->done_seq, 0};
            p->solo_left = 0;
            HIP_TRY(hipMemcpy(p->d_dev, init, sizeof init, hipMemcpyHostToDevice));
            *(volatile int*)p->go_flag = 0;         // (an earlier call that gave a launch up left -1 here)
        }
        return FRL_OK;
    }
    int join_alt() {              // work for the engine's stream that is not part of the doorbell protocol: stream2 drained first
        if (arm.alt_busy) { HIP_TRY(hipStreamSynchronize(p->stream2)); arm.alt_busy = false; }
        arm.on_alt = false;
        return FRL_OK;
    }

    // ---- 1. this step's actions: from the previous step's launch ...
    int wait_actions() {
        if (!act.on_host) HIP_TRY(hipMemcpyAsync(p->env_act, p->d_env, (size_t)n * plan.aout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        bool seen = false;
        if (act.flagged) {               // spin on the pinned word for up to ~2 s, then fall back to the stream
            volatile int* fl = p->done_flag;
            const auto t_spin = std::chrono::steady_clock::now();
            for (long long it = 0; !seen; ++it) {
                if (*fl == act.expect_done) { seen = true; break; }
                if ((it & 0xfff) == 0xfff && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_spin).count() > 2.0) break;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        }
        if (!seen) {
            if (arm.alt_busy) { HIP_TRY(hipStreamSynchronize(p->stream2)); arm.alt_busy = false; }
            HIP_TRY(hipStreamSynchronize(e->stream));
            FRL_TRY(solo_err_check(e));     // (a launch that gave up left no actions: do not step the envs on the old ones)
        }
        return FRL_OK;
    }
    // (what an act launch is told about exploration: the separate launch and the solo tail — exactly what the separate act launch of the
    // next step would be given)
    ActExplore explore_args() const {
        ActExplore ex;
        ex.x.kind = plan.kind; ex.x.epsilon = ra->epsilon; ex.x.sigma = ra->explore_sigma; ex.x.scale = 1.f; ex.x.max_action = plan.ma;
        ex.x.ou_theta = ra->ou_theta; ex.x.ou_sigma = ra->ou_sigma; ex.x.ou_dt = ra->ou_dt;
        ex.scale_dev = ra->max_episodes > 0 ? in.scale : nullptr;      // the last block: in place in pinned memory, or its upload
        ex.ou_state_dev = p->d_ou; ex.flags_dev = in.flags; ex.env_out_dev = env_out;
        ex.device_eps = true;
        return ex;
    }
    // ... from a separate act launch on the device-resident observations, exploration included ...
    int act_device() {
        const ActExplore ex = explore_args();
        const size_t bytes = (size_t)n * plan.aout * sizeof(float);
        FRL_TRY(join_alt());
        FRL_TRY(launch_act(e, 0, plan.mode, 0, 0, E, O, p->d_obs_cur, nullptr, p->d_store, nullptr, &ex));
        if (!plan.zero_copy) HIP_TRY(hipMemcpyAsync(p->env_act, p->d_env, bytes, hipMemcpyDeviceToHost, e->stream));
        if (plan.host_commit && plan.mode != FRL_ACT_ARGMAX) HIP_TRY(hipMemcpyAsync(p->act_out, p->d_store, bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return FRL_OK;
    }
    // ... or round 1's way: obs up, policy output down, exploration by the host generator
    int act_host() {
        const bool dqn = plan.mode == FRL_ACT_ARGMAX, sac = plan.mode == FRL_ACT_SAC_SAMPLE;
        const float ma = plan.ma;
        HIP_TRY(hipMemcpyAsync(p->d_obs, p->obs, (size_t)n * O * sizeof(float), hipMemcpyHostToDevice, e->stream));
        if (sac) {
            for (size_t i = 0; i < (size_t)n * A; ++i) p->eps[i] = (float)p->host_rng.normal();
            HIP_TRY(hipMemcpyAsync(p->d_eps, p->eps, (size_t)n * A * sizeof(float), hipMemcpyHostToDevice, e->stream));
        }
        FRL_TRY(launch_act(e, 0, plan.mode, 0, 0, E, O, p->d_obs, sac ? p->d_eps : nullptr, p->d_out, nullptr));
        HIP_TRY(hipMemcpyAsync(p->act_out, p->d_out, (size_t)n * plan.aout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        // exploration (host generator): epsilon-greedy (DQN.py:307-310) / Gaussian action noise (TD3.py:412)
        for (int i = 0; i < n; ++i) {
            if (dqn) {
                float a = p->act_out[i];
                if (p->host_rng.uniform() < ra->epsilon) a = (float)(int)(p->host_rng.uniform() * p->pool->spec.n_actions);
                p->act_out[i] = a;
                p->env_act[i] = a;
            } else {
                const float sc = plan.kind == FRL_EXPLORE_GAUSS ? decayed_scale(ra, p->pool, i / E, E) * ra->explore_sigma : 0.f;
                for (int c = 0; c < A; ++c) {
                    float v = p->act_out[(size_t)i * A + c] * ma;
                    if (sc > 0.f) v += sc * ma * (float)p->host_rng.normal();
                    p->env_act[(size_t)i * A + c] = v < -ma ? -ma : (v > ma ? ma : v);
                }
            }
        }
        return FRL_OK;
    }
    // ---- 2. the envs step: into the block (device path) or into the pool's own staging
    int env_step() {
        nobs = plan.dev ? host.next_obs : p->next_obs;
        onext = plan.dev ? host.obs_next : p->obs_next;
        rew = plan.dev ? host.reward : p->reward;
        p->pool->step(p->env_act, nobs, rew, p->term, p->trunc, onext);
        lap(1);
        return p->pool->cb_error ? fail(FRL_ERR_STATE, "env step callback failed (%d)", p->pool->cb_error) : (int)FRL_OK;
    }
    // ---- 3. host_commit: add(obs, action, reward, next_obs, terminated) through the stage
    int stage_records() {
        const int aout = plan.aout;
        const float* stored = (plan.dev && plan.mode == FRL_ACT_ARGMAX) ? p->env_act : p->act_out;       // DQN stores the explored index
        for (int i = 0; i < n; ++i) {
            float* r = rec.data();
            std::memcpy(r + h.rec.obs_off[0], p->obs + (size_t)i * O, sizeof(float) * O);
            std::memcpy(r + h.rec.act_off[0], stored + (size_t)i * aout, sizeof(float) * aout);
            r[h.rec.rew_off] = rew[i];
            r[h.rec.done_off] = p->term[i] ? 1.f : 0.f;
            std::memcpy(r + h.rec.nobs_off[0], nobs + (size_t)i * O, sizeof(float) * O);
            FRL_TRY(stage_one(e, i / E, r));
        }
        return FRL_OK;
    }
    // ---- 4. the rest of the block: flags, ring rows, the learners' noise multipliers.  Returns the smallest ring's size with this step's rows in
    int fill_block() {
        for (int i = 0; i < n; ++i) {
            const int q = i / E;
            host.flags[i] = (unsigned char)((p->term[i] ? 1 : 0) | ((p->term[i] || p->trunc[i]) ? 2 : 0));
            if (!plan.host_commit) {                     // Buffer.add's cursor arithmetic (Buffer.py:36-38), the row written on the device
                host.row[i] = e->index[q];
                e->index[q] = (e->index[q] + 1) % h.capacity;
                if (e->size[q] < h.capacity) e->size[q]++;
            }
        }
        for (int q = 0; q < h.P; ++q) host.scale[q] = decayed_scale(ra, p->pool, q, E);
        act.have_action = false;
        return min_ring_size();
    }

    // ---- 5a. a learn step on the fold: add(), learn() and the next select_action + exploration in the learn launches
    // The armed launch is told to give up: -1 in the doorbell, BOTH streams drained (the launch may sit on either), and every counter the
    // arming advanced put back — the engine's Philox counters and TD3's policy-delay phase are where a plain step would have left them
    // (also after a recovered env exception: the destructor).  Silent: the caller says what a failed drain means
    hipError_t cancel_armed() {
        std::atomic_thread_fence(std::memory_order_release);
        *(volatile int*)p->go_flag = -1;
        hipError_t he = hipStreamSynchronize(p->stream2);
        const hipError_t he1 = hipStreamSynchronize(e->stream);
        if (he == hipSuccess) he = he1;
        e->rng_counter = arm.rng; e->param_version = arm.pver; e->solo_bar_base = arm.bar; p->total_it = arm.total_it;
        p->done_seq = arm.done_seq; p->go_seq = arm.go_seq; p->solo_left = arm.solo_left; arm.on_alt = arm.was_on_alt;
        *(volatile int*)p->go_flag = 0;
        arm.armed = arm.alt_busy = false;
        return he;
    }
    // One folded launch in the making: the variant's builder fills its argument struct and advances what the arguments take (go_seq, done_seq,
    // total_it), the skeleton launches.  act: the launch also selects the next step's actions (0 on the call's last step); left: workgroups
    // the step adds to the solo "have left" count
    struct StepLaunch {
        int act, done_value = 0, left = 0;
        bool flagged, armed;
        frl_learn_args la;
        DqnStepArgs dqn;
        SoloStepArgs solo;
        StepFold fold;
    };
    // DQN (kernels_dqn2.hip): commit, update and epsilon-greedy act are one launch; an armed one waits for the done value of the launch in front
    int dqn_step_args(StepLaunch& s) {
        DqnStepArgs& sa = s.dqn;
        memset(&sa, 0, sizeof sa);
        sa.commit = 1; sa.act = s.act;
        sa.E = E; sa.O = O;
        sa.obs_cur = p->d_obs_cur; sa.store_act = p->d_store;
        set_sections(sa, in);
        sa.act_out = p->d_store; sa.env_out = env_out;
        if (s.armed) { sa.go_flag = go_dev; sa.go_value = ++p->go_seq; sa.dev_wait = p->done_seq; }
        if (s.flagged) { sa.done_flag = flag_dev; sa.done_value = ++p->done_seq; if (plan.prearm) sa.dev_done = p->d_dev; }
        if (s.armed) { sa.dev_done = p->d_dev; sa.err = e->d_solo_err; }
        sa.epsilon = ra->epsilon;
        sa.act_counter = e->rng_counter + 1;    // learn() takes the next counter value, the act draw the one after (as separate launches do)
        ++p->total_it;
        s.fold.dqn = &sa; s.done_value = sa.done_value;
        return FRL_OK;
    }
    // DDPG / TD3 / SAC (kernels_solo.hip): add() at the head of the critic launch, the act at the tail of the step's last launch (the actor launch
    // on TD3's policy steps); an armed one waits for the count of workgroups that have left
    int solo_step_args(StepLaunch& s) {
        SoloStepArgs& ss = s.solo;
        memset(&ss, 0, sizeof ss);
        ss.act = s.act;
        ss.c.obs_cur = p->d_obs_cur; ss.c.store_act = p->d_store;
        set_sections(ss.c, in);
        ss.c.n = n; ss.c.E = E; ss.c.O = O; ss.c.aout = plan.aout;
        if (ss.act) {
            const ActExplore ex = explore_args();
            FRL_TRY(launch_act(e, 0, plan.mode, 0, 0, E, O, p->d_obs_cur, nullptr, p->d_store, nullptr, &ex, &ss.act_args));
            ss.act_args.rng_counter = e->rng_counter + 1;      // learn() takes the next counter value, the act draw the one after (as separate launches do)
        }
        ss.ticket = e->d_solo_ticket;
        ss.bar2 = e->d_solo_bar + (size_t)h.P * kSoloWG;
        if (s.flagged) { ss.done_flag = flag_dev; ss.done_value = ++p->done_seq; }
        if (s.armed) { ss.go_flag = go_dev; ss.go_value = ++p->go_seq; ss.dev_wait = p->solo_left; }
        if (plan.prearm) ss.dev_cnt = p->d_dev + 1;
        ++p->total_it;
        if (h.algo == ALGO_TD3) s.la.do_actor = (ra->policy_freq <= 1) || (p->total_it % ra->policy_freq == 0);
        s.left = h.P * h.solo * ((h.algo == ALGO_TD3 && !s.la.do_actor) ? 1 : 2);
        s.fold.solo = &ss; s.done_value = ss.done_value;
        return FRL_OK;
    }
    // the step's launch: arguments of vector step `st` (this one, or — armed — the next one, whose rings hold size_at_launch rows by then)
    int launch_step(int st, int size_at_launch, bool armed) {
        StepLaunch s;
        s.act = (st + 1 < ra->n_steps) ? 1 : 0; s.flagged = plan.poll && s.act; s.armed = armed;
        s.la = ra->learn; s.la.stats_out = nullptr;
        s.fold = StepFold{nullptr, nullptr, size_at_launch, nullptr};
        if (armed) {            // what arming is about to advance
            arm.rng = e->rng_counter; arm.pver = e->param_version; arm.bar = e->solo_bar_base; arm.total_it = p->total_it;
            arm.done_seq = p->done_seq; arm.go_seq = p->go_seq; arm.solo_left = p->solo_left; arm.was_on_alt = arm.on_alt;
            arm.t = std::chrono::steady_clock::now();
        }
        FRL_TRY(plan.fold == FOLD_DQN ? dqn_step_args(s) : solo_step_args(s));
        if (!armed) FRL_TRY(join_alt());
        s.fold.stream = armed && !arm.on_alt ? p->stream2 : nullptr;
        FRL_TRY(learn_impl(e, &s.la, &s.fold));
        if (armed) { arm.on_alt = (s.fold.stream != nullptr); arm.alt_busy = arm.alt_busy || arm.on_alt; }
        p->solo_left += s.left;
        if (s.act) e->rng_counter++;
        if (armed) { arm.armed = true; arm.armed_act = s.act != 0; arm.armed_done = s.done_value; }
        else { act.have_action = s.act != 0; act.on_host = plan.zero_copy; act.flagged = s.flagged; act.expect_done = s.done_value; }
        return FRL_OK;
    }
    int folded_step(int step) {
        bool rung = false;
        if (arm.armed) {                // this step's launch is already there, spinning, and the block is complete
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - arm.t).count() >= plan.arm_patience) {      // ... too late: the step is launched below
                const hipError_t he = cancel_armed();
                if (he != hipSuccess) return fail(FRL_ERR_HIP, "cancelling a pre-armed launch: %s", hipGetErrorString(he));
            } else {                    // -> ring the doorbell
                std::atomic_thread_fence(std::memory_order_release);
                *(volatile int*)p->go_flag = p->go_seq;
                arm.armed = false;
                act.have_action = arm.armed_act; act.on_host = true; act.flagged = arm.armed_act; act.expect_done = arm.armed_done;
                rung = true;
            }
        }
        if (!rung) {
            if (!plan.zero_copy) HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->lay.bytes, hipMemcpyHostToDevice, e->stream));
            FRL_TRY(launch_step(step, -1, false));
        }
        updates += h.P;
        std::memcpy(p->obs, onext, sizeof(float) * (size_t)n * O);
        if (plan.prearm && step + 1 < ra->n_steps) {          // the next step's launch, now: will it be a learn step?
            const int msz1 = min_ring_size(E);
            if (learn_due(*ra, step + 1, msz1)) FRL_TRY(launch_step(step + 1, msz1, true));
        }
        return FRL_OK;
    }
    // ---- 5b. every other step: the commit on its own ...
    int plain_commit() {
        if (!plan.dev) { std::swap(p->obs, p->obs_next); p->dev_obs_valid = false; return FRL_OK; }
        FRL_TRY(join_alt());
        if (plan.host_commit) {                          // the records went through the stage; the device still needs obs_next and the flags
            HIP_TRY(hipMemcpyAsync(p->d_blk, p->blk, p->lay.bytes, hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(p->d_obs_cur, p->d_blk + p->lay.off_onext, (size_t)n * O * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
        } else {
            FRL_TRY(rollout_commit(e, p, E, plan.aout, nullptr, 0, blk_dev));
        }
        std::memcpy(p->obs, onext, sizeof(float) * (size_t)n * O);          // host mirror of what the policy sees next
        return FRL_OK;
    }
    // ... and, where one is due, frl_learn (a PER engine: between its sample and its priority update)
    int plain_learn(int step) {
        if (!learn_due(*ra, step, min_ring_size())) return FRL_OK;
        frl_learn_args la = ra->learn;
        la.stats_out = nullptr;
        ++p->total_it;
        if (h.algo == ALGO_TD3) la.do_actor = (ra->policy_freq <= 1) || (p->total_it % ra->policy_freq == 0);
        if (la.per) FRL_TRY(frl_per_sample(e, la.batch, nullptr, nullptr, nullptr));
        FRL_TRY(frl_learn(e, &la));
        if (la.per) FRL_TRY(frl_per_update(e, la.batch, nullptr, nullptr));
        updates += h.P;
        return FRL_OK;
    }
    int close() {
        FRL_TRY(join_alt());
        FRL_TRY(flush_stage(e));
        HIP_TRY(hipStreamSynchronize(e->stream));
        FRL_TRY(solo_err_check(e));
        if (plan.timing && ra->n_steps > 0)
            fprintf(stderr, "frl_rollout: per vector step  act + readback (waits for the learn) %.1f us, env step %.1f us, block + commit %.1f us, learn launches %.1f us\n",
                    t_sec[0] / ra->n_steps * 1e6, t_sec[1] / ra->n_steps * 1e6, t_sec[2] / ra->n_steps * 1e6, t_sec[3] / ra->n_steps * 1e6);
        return FRL_OK;
    }
};

// The rollout-and-update loop for a population, mirroring the reference loop's per-step order (select_action,
// exploration, env.step, add, learn; DQN.py:294-339, TD3.py:403-450, SAC.py:519-566) for P learners x E env instances
// at once.  Per vector step (host_explore = 0):
//   act launch on the device-resident observations, exploration included (Philox)  -D2H env actions->
//   env workers step  -H2D one block: next_obs, obs_next, reward, flags, ring rows, per-learner noise scale->
//   commit launch (records assembled from device-resident obs / actions + the block)  ->  frl_learn (device sampling)
// host_explore = 1 is round 1's loop: obs H2D, action D2H, exploration by a host generator, records staged from the host.
// Which calls are refused and which of these paths a call takes: plan_rollout (rollout_plan.hpp).
extern "C" int frl_rollout(frl_engine* e, frl_envpool* p, const frl_rollout_args* ra, frl_rollout_stats* out) {
    ENG(e);
    const AlgoTraits& T = algo_traits(e->h.algo);
    if (*T.act_hint) return wrong_engine(e->h, "frl_rollout");      // (no fused collection where the explore launch does not serve; said before the arguments are looked at, as ever)
    if (!p || !ra) return fail(FRL_ERR_INVALID, "NULL argument");
    if (!T.rollout) return wrong_engine(e->h, "frl_rollout");
    RolloutPlan plan;
    std::string why;
    const int refused = plan_rollout(rollout_facts(e, p, ra->learn.batch), rollout_knobs(), *ra, &plan, &why);
    if (refused) return fail(refused, "%s", why.c_str());
    RolloutTally tally;
    FRL_TRY(rollout_begin(e, p, plan.aout, plan.dev, &tally));
    RolloutRun run(e, p, ra, plan);
    FRL_TRY(run.open(&tally));
    for (int step = 0; step < ra->n_steps; ++step) {
        FRL_TRY(!plan.dev ? run.act_host() : run.act.have_action ? run.wait_actions() : run.act_device());
        run.lap(0);
        FRL_TRY(run.env_step());
        if (plan.host_commit) FRL_TRY(run.stage_records());
        const int min_size = plan.dev ? run.fill_block() : 0;
        const bool folded = plan.fold != FOLD_NONE && learn_due(*ra, step, min_size);
        FRL_TRY(folded ? run.folded_step(step) : run.plain_commit());
        run.lap(2);
        if (!folded) FRL_TRY(run.plain_learn(step));
        run.lap(3);
    }
    FRL_TRY(run.close());
    rollout_finish(p, tally, (long long)ra->n_steps * run.n, run.updates, out);
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
    RolloutTally tally;
    FRL_TRY(rollout_begin(e, p, stored, true, &tally));
    const int mode = disc ? FRL_ACT_CAT_SAMPLE : FRL_ACT_PPO_SAMPLE;
    const float ma = disc ? 1.f : es.max_action;
    const int n_mb = (T + ra->learn.minibatch - 1) / ra->learn.minibatch;
    long long updates = 0;
    const BlkView b = p->lay.view(p->blk);
    HIP_TRY(hipStreamSynchronize(e->stream));
    tally.t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < ra->n_iters; ++it) {
        for (int t = 0; t < Tseg; ++t) {
            // Normal.sample(): mean + std * N(0,1) (:240-242); Categorical.sample(): argmax(p / q), q ~ Exp(1) (:249-251) — the
            // variates come from the launch's Philox stream; action_ = clip(action * max_action) (:529-530) in the same launch
            ActExplore ex;
            ex.x.kind = FRL_EXPLORE_NONE; ex.x.max_action = ma; ex.x.scale = 1.f;
            ex.env_out_dev = p->d_env; ex.device_eps = true;
            FRL_TRY(launch_act(e, 0, mode, 0, 0, E, O, p->d_obs_cur, nullptr, p->d_store, p->d_logp, &ex));
            HIP_TRY(hipMemcpyAsync(p->env_act, p->d_env, (size_t)n * stored * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            p->pool->step(p->env_act, b.next_obs, b.reward, p->term, p->trunc, b.obs_next);
            if (p->pool->cb_error) return fail(FRL_ERR_STATE, "env step callback failed (%d)", p->pool->cb_error);
            for (int i = 0; i < n; ++i) {     // add(obs, action, reward, next_obs, terminated, log_pi, done): flags + the ring row
                const bool ended = p->term[i] || p->trunc[i];
                b.flags[i] = (unsigned char)((p->term[i] ? 1 : 0) | (ended ? 2 : 0) | ((ended || t == Tseg - 1) ? 4 : 0));
                b.row[i] = (i % E) * Tseg + t;                       // env j's segment is contiguous in the ring
            }
            FRL_TRY(rollout_commit(e, p, E, stored, p->d_logp, stored));
        }
        std::memcpy(p->obs, b.obs_next, sizeof(float) * (size_t)n * O);
        for (int q = 0; q < h.P; ++q) { e->index[q] = T % h.capacity; e->size[q] = T; }
        FRL_TRY(frl_ppo_learn(e, &ra->learn));
        updates += (long long)h.P * ra->learn.k_epochs * n_mb;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    rollout_finish(p, tally, (long long)ra->n_iters * Tseg * n, updates, out);
    return FRL_OK;
}
