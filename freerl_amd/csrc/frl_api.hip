// Host side of the C ABI (include/freerl_hip.h): engine construction, the replay ring's pinned
// staging, parameter import/export, kernel launches.  Compiled with hipcc for gfx950 only.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/freerl_hip.h"
#include "frl_desc.h"
#include "engine_plan.hpp"
#include "her_plan.h"
#include "host_mem.hpp"

#include "kernels.h"
#ifdef FRL_UNITY      // developer variants (tools/phase_timing.py): one translation unit, so that the phase-timing symbols exist once
#include "kernels_replay.hip"
#include "kernels_update.hip"
#include "kernels_dqn.hip"
#include "kernels_critic.hip"
#include "kernels_actor.hip"
#include "kernels_act.hip"
#include "kernels_ppo.hip"
#include "kernels_ppo2.hip"
#include "kernels_critic2.hip"
#include "kernels_actor2.hip"
#include "kernels_criticw.hip"
#include "kernels_actorw.hip"
#include "kernels_criticx.hip"
#include "kernels_actorx.hip"
#include "kernels_dqn2.hip"
#include "kernels_per.hip"
#include "kernels_noisy.hip"
#include "kernels_c51.hip"
#include "kernels_solo.hip"
#include "kernels_solow.hip"
#include "kernels_sacd.hip"
#include "kernels_reinforce.hip"
#include "kernels_envelope.hip"
#include "kernels_envelope_ddpg.hip"
#include "kernels_gail.hip"
#include "kernels_gail_ppo.hip"
#include "kernels_mappo.hip"
#include "kernels_happo.hip"
#include "kernels_mappo_mask.hip"
#include "kernels_mappo_state.hip"
#include "kernels_att.hip"
#include "kernels_masac.hip"
#include "kernels_her.hip"
#include "kernels_cem_gd3pg.hip"
#endif

using namespace frl;

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(FRL_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

struct HipMem {                   // host_mem.hpp's backend.  hipFree synchronises the device: what makes regrowing a buffer under a busy stream safe
    using error_t = hipError_t;
    using stream_t = hipStream_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t device_free(void* p) { return hipFree(p); }
    static hipError_t pinned_alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static hipError_t pinned_free(void* p) { return hipHostFree(p); }
    static hipError_t memset_async(void* p, int value, size_t bytes, hipStream_t s) { return hipMemsetAsync(p, value, bytes, s); }
};
using HostMem = frl::MemOwner<HipMem>;

// developer / test knobs from the environment, read where they are used (most of them per call).  Three meanings, kept apart:
// env_set: the variable is set at all; env_flag(name, false): set and nonzero; env_flag(name, true): a default-on path that "=0" switches off
static bool env_set(const char* name) { return getenv(name) != nullptr; }
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static bool env_flag(const char* name, bool dflt) { const char* v = getenv(name); return v ? atoi(v) != 0 : dflt; }
static double env_double(const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; }

// (LearnFamily, the kernel family an engine's frl_learn() runs on: engine_plan.hpp; frl_api_learn.inc registers each family's kernels)
using LearnKernel = void (*)(const frl::EngineDesc*, frl::LearnArgs);
using SolowKernel = void (*)(const frl::EngineDesc*, frl::LearnArgs, frl::SoloArgs);
using SoloKernel = void (*)(const frl::EngineDesc*, frl::LearnArgs, frl::SoloArgs, frl::SoloStepArgs);
using DqnKernel = void (*)(const frl::EngineDesc*, frl::LearnArgs, frl::DqnStepArgs);
using RowKernel = void (*)(const frl::EngineDesc*, frl::LearnArgs, int);      // the row-chunk launch shape: (unit, slab) workgroups, ns slabs per unit
struct KernelPtr {                // one typed member per kernel signature; a family uses the one its kernels have
    LearnKernel k = nullptr;
    SolowKernel kw = nullptr;
    SoloKernel ks = nullptr;
    DqnKernel kd = nullptr;
    RowKernel kr = nullptr;
    KernelPtr() = default;
    KernelPtr(RowKernel f) : kr(f) {}
    KernelPtr(LearnKernel f) : k(f) {}
    KernelPtr(SolowKernel f) : kw(f) {}
    KernelPtr(SoloKernel f) : ks(f) {}
    KernelPtr(DqnKernel f) : kd(f) {}
    const void* address() const { return k ? (const void*)k : kw ? (const void*)kw : ks ? (const void*)ks : kd ? (const void*)kd : (const void*)kr; }
};
struct LearnKernels {             // a family's kernels for one engine's shape (resolve_learn_kernels)
    KernelPtr critic, critic_nv, actor, step;
    int lds_bytes = 0, block = 256;
};

// An entry point called on an engine of an algorithm it does not serve: the call, the algorithm and the entry point that updates it
static int wrong_engine(const EngineDesc& h, const char* who, int code = FRL_ERR_STATE) {
    const AlgoTraits& T = algo_traits(h.algo);
    return fail(code, "%s does not serve %s engines (updates: %s)%s%s%s", who, T.name, *T.learn ? T.learn : "none",
                *T.act_hint ? "; such an engine acts through frl_act (" : "", T.act_hint, *T.act_hint ? ")" : "");
}

struct frl_engine : frl::EngineFacts {      // (what the plan fixed: family, lds_bytes, has_nets, the buffer sizes, n_cus — engine_plan.hpp)
    HostMem mem;                  // owns every device and pinned buffer below and in h: allocate through it and frl_destroy needs no line
    frl_config cfg;
    EngineDesc h;                 // host mirror of the device descriptor
    EngineDesc* d = nullptr;      // device copy
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_stage = nullptr;
    LearnKernels kern;                    // the kernels of the engine's family (a DQN engine: the one-launch update's)
    // replay cursors (host authoritative, reference semantics Buffer.py:23-24,36-38): [n_rings][P], ring 0's first
    std::vector<int> index, size;
    // pinned staging of not-yet-flushed adds
    float* stage_rows = nullptr;          // [stage_cap][width] pinned
    long long* stage_slots = nullptr;     // [stage_cap] pinned
    float* d_stage_rows = nullptr;
    long long* d_stage_slots = nullptr;
    int stage_cap = 0, stage_n = 0;
    bool stage_inflight = false;
    std::vector<int> staged_per_learner;  // rows staged since the last flush (a flush may not hold one ring row twice)
    // pinned scratch for idx / noise uploads
    int* h_idx = nullptr;
    long long* h_idx64 = nullptr;
    long long* d_idx64 = nullptr;
    float* h_noise = nullptr;
    unsigned long long rng_counter = 0;
    // act scratch (device)
    // [slot][P][net size]: fragment-image nets re-laid out to Wk for act_kernel (wide chained engines), one slot per
    // (net, online | target), sized once at frl_create; a slot is re-laid out only when the engine's parameters have changed since
    // (param_version: bumped by frl_learn, frl_params_set and the obs-norm relayout)
    float* d_act_wk = nullptr;
    std::vector<unsigned long long> act_wk_version;   // [2 * n_nets], 0 = never laid out
    unsigned long long param_version = 1;
    // kernels_solo.hip (h.solo): per-workgroup gradient slabs, partial sums, the learners' grid-barrier counters
    float* d_solo_slab = nullptr;
    float* d_solo_part = nullptr;
    unsigned* d_solo_bar = nullptr;
    int* d_solo_err = nullptr;            // device address of h_solo_err
    int* d_solo_pre = nullptr;            // [2][P][kSoloPre]: the next call's rows, drawn a launch ahead (SoloArgs::pre_read / pre_write)
    unsigned solo_pre_seq = 0;            // critic-stage launches so far: which of the two slots is read / written
    // kernels_solow.hip, multi-agent: what the rows in the slot the next launch reads were drawn for (the HOST decides whether draw_kernel runs)
    bool ma_pre_valid = false;
    unsigned long long ma_pre_counter = 0;
    int ma_pre_size = 0, ma_pre_batch = 0;
    int* h_solo_err = nullptr;            // pinned: a solo workgroup that waited 2 s for its learner's others sets it (checked after syncs: solo_err_check)
    int* d_solo_ticket = nullptr;         // the rollout tail's learner ticket
    unsigned solo_bar_base = 0;           // arrivals every counter has seen (one counting barrier per launch: kSoloWG)
    unsigned* d_solow_bar2 = nullptr;     // [units][64] "critic stepped" flags of the helper workgroups (the fused policy step)
    float* d_act_in = nullptr;
    float* d_act_eps = nullptr;
    float* d_act_out = nullptr;
    float* d_act_logp = nullptr;
    size_t act_in_cap = 0, act_eps_cap = 0, act_out_cap = 0, act_logp_cap = 0;      // floats each holds (act_scratch)
    float* d_ou = nullptr;                // frl_act_explore's Ornstein-Uhlenbeck state [P][n_rows][A]
    unsigned char* d_ou_flags = nullptr;
    size_t ou_n = 0;
    // ppo scratch
    float* d_ppo = nullptr;
    size_t ppo_cap = 0;
    int* d_perm = nullptr;
    size_t perm_cap = 0;
    float* h_noisy = nullptr;             // pinned staging for uploaded noise
    // prioritised replay (frl_per_*): sum-tree + max-tree per learner, float64 like the reference's SumTree
    bool per_on = false;
    double* d_per_sum = nullptr;
    double* d_per_max = nullptr;
    float per_alpha = 0.5f, per_eps = 0.01f;
    double per_beta = 0.4, per_beta_inc = 0.001;
    std::vector<int> bucket_cursor;
    std::vector<int> size_flushed;        // rows valid per learner as of the last flush (PER_Buffer.add's `len(self.buffer) == 0`)
    // frl_reinforce_learn: the learners' row counts of a call, staged in two alternating pinned slots (the call does not wait for the stream)
    int* h_ep_n = nullptr;                // [2][P] pinned
    hipEvent_t ev_ep[2] = {nullptr, nullptr};
    unsigned ep_seq = 0;
    float* h_gail_rows = nullptr;         // frl_gail_learn: pinned staging of the uploaded policy rows [P][batch_max][obs_dim + act_dim]
    float* h_cem_ctl = nullptr;           // frl_cem_gd3pg_learn: pinned staging of EngineDesc::cem_ctl, two alternating slots [2][2][P] (ev_ep, ep_seq: as h_ep_n)
    float* h_env_w = nullptr;             // frl_envelope_learn / frl_envelope_ddpg_learn: pinned staging of uploaded preference vectors [P][batch_max][reward_dim]
    // frl_her_relabel: the call's small arrays in one pinned block and its device copy (both grow on demand), the event behind the copy
    unsigned char* h_her = nullptr;
    unsigned char* d_her = nullptr;
    size_t her_cap_h = 0, her_cap_d = 0;
    hipEvent_t ev_her = nullptr;
    bool her_inflight = false;
    unsigned long long her_calls = 0;     // relabel calls that drew on the device: the Philox counter of the next one
    int* d_size = nullptr;                // [2][P]: size before the flush being applied / current size
    int* stage_bucket = nullptr;          // PER, pinned: [off[P + 1] | size_before[P] | leaf[stage_cap]] of the flush being applied
    int* d_stage_bucket = nullptr;
    float* d_per_prio = nullptr;          // [P][batch_max] float32 priorities of the last sample
    double* d_uniforms = nullptr;         // [P][batch_max]
    // optional per-kernel timing (frl_profile_*): event pairs recorded around each launch
    bool profile = false;
    std::vector<hipEvent_t> prof_ev;      // pool, pairs
    std::vector<int> prof_kind;           // kernel kind per recorded pair
    size_t prof_used = 0;
    double prof_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long prof_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

enum ProfKind { PK_DRAW = 0, PK_GRAD_CRITIC = 1, PK_ADAM_CRITIC = 2, PK_GRAD_ACTOR = 3, PK_ADAM_ACTOR = 4, PK_SOFT = 5, PK_PPO = 6 };

static void prof_begin(frl_engine* e, int kind) {
    if (!e->profile) return;
    if (e->prof_used + 2 > e->prof_ev.size()) {
        for (int i = 0; i < 2; ++i) { hipEvent_t ev; hipEventCreate(&ev); e->prof_ev.push_back(ev); }
    }
    hipEventRecord(e->prof_ev[e->prof_used], e->stream);
    e->prof_kind.push_back(kind);
}
static void prof_end(frl_engine* e) {
    if (!e->profile) return;
    hipEventRecord(e->prof_ev[e->prof_used + 1], e->stream);
    e->prof_used += 2;
}
static void prof_collect(frl_engine* e) {
    if (e->prof_used == 0) return;
    hipStreamSynchronize(e->stream);
    for (size_t i = 0; i < e->prof_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->prof_ev[i], e->prof_ev[i + 1]) == hipSuccess) {
            const int k = e->prof_kind[i / 2];
            e->prof_ms[k] += ms;
            e->prof_n[k]++;
        }
    }
    e->prof_used = 0;
    e->prof_kind.clear();
}

// --------------------------------------------------------------------------------- lifetime
extern "C" const char* frl_last_error(void) { return g_err.c_str(); }
extern "C" int frl_version(void) { return 114; }      // 101: frl_rollout_args.explore_kind 0 = FRL_EXPLORE_DEFAULT; 102: frl_learn_work_executed; 103: frl_config.reward_dim (appended), frl_envelope_learn; 104: FRL_ALGO_ENVELOPE_DDPG, frl_envelope_ddpg_learn; 105: FRL_ALGO_GAIL, FRL_ACT_LEAKY_RELU, frl_gail_learn, frl_gail_reward; 106: FRL_ALGO_MAPPO, FRL_ALGO_IPPO, frl_mappo_learn, frl_net_norm_set; 107: FRL_ALGO_HAPPO, frl_happo_args, frl_happo_learn; 108: frl_action_mask_set, frl_act_masked; 109: frl_config_ext, frl_create_ex, frl_state_info (the level whose body read `return 109;`: tests/test_mappo_state_abi.py looks for that text in this file); 110: FRL_ALGO_MADDPG_ATT (likewise `return 110;`: tests/test_att_abi.py); 111: FRL_ALGO_MASAC, frl_alpha_get_agent, frl_alpha_set_agent; 112: frl_her_args, frl_her_relabel; 113: FRL_ALGO_GAIL_PPO, frl_gail_ppo_args, frl_gail_ppo_learn, frl_log_std_range_set / _get; 114: FRL_ALGO_CEM_GD3PG, frl_cem_gd3pg_args, frl_cem_gd3pg_learn, frl_ring_add / _add_batch / _cursor_get / _cursor_set

extern "C" int frl_device_count(int* n_out) {
    if (!n_out) return fail(FRL_ERR_INVALID, "n_out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *n_out = 0; return fail(FRL_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n_out = n;
    return FRL_OK;
}

extern "C" int frl_destroy(frl_engine* e) {
    if (!e) return FRL_OK;
    hipSetDevice(e->cfg.device_id);
    if (e->stream) hipStreamSynchronize(e->stream);
    e->mem.release_all();
    for (hipEvent_t ev : e->ev_ep) if (ev) hipEventDestroy(ev);
    for (hipEvent_t ev : {e->ev0, e->ev1, e->ev_stage, e->ev_her}) if (ev) hipEventDestroy(ev);
    for (hipEvent_t ev : e->prof_ev) hipEventDestroy(ev);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
    return FRL_OK;
}

static LearnKernels resolve_learn_kernels(LearnFamily fam, int chain_waves, bool actor_park, const EngineDesc& h);
static hipError_t set_family_lds_attributes(LearnFamily fam);

extern "C" int frl_create(const frl_config* cfg, frl_engine** out) { return frl_create_ex(cfg, nullptr, out); }

// the developer / test knobs that are read once, at create, for plan_engine (every other knob is read where it is used, per call)
static PlanKnobs create_knobs() {
    auto tri = [](const char* name) { return env_set(name) ? (int)env_flag(name, false) : -1; };
    PlanKnobs k;
    k.assume_cus = env_int("FRL_ASSUME_CUS", k.assume_cus);
    k.rc = env_int("FRL_RC", k.rc);
    k.cps = env_int("FRL_CPS", k.cps);
    k.solow_narrow = env_flag("FRL_SOLOW_NARROW", k.solow_narrow);
    k.critic_v2 = tri("FRL_CRITIC_V2");
    k.solo = tri("FRL_SOLO");
    k.solo_maxp = env_int("FRL_SOLO_MAXP", k.solo_maxp);
    k.solow = tri("FRL_SOLOW");
    k.solow_helpers = env_flag("FRL_SOLOW_HELPERS", k.solow_helpers);
    k.chain_waves = env_int("FRL_CHAIN_WAVES", k.chain_waves);
    k.actor_park = env_flag("FRL_ACTOR_PARK", k.actor_park);
    return k;
}

// ext: what frl_config cannot grow to hold (its last field is pinned).  NULL, or state_dim 0: frl_create's engine exactly
extern "C" int frl_create_ex(const frl_config* cfg, const frl_config_ext* ext, frl_engine** out) {
    if (!cfg || !out) return fail(FRL_ERR_INVALID, "cfg/out is NULL");
    *out = nullptr;
    const frl_config& c = *cfg;
    std::string why;
    if (const int rc = check_create_args(c, ext, &why)) return fail(rc, "%s", why.c_str());
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(FRL_ERR_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (c.device_id < 0 || c.device_id >= ndev) return fail(FRL_ERR_INVALID, "device_id %d of %d", c.device_id, ndev);
    HIP_TRY(hipSetDevice(c.device_id));
    PlanLimits limits;      // what the device can hold resident at once: the solo kernels' flag hand-overs spin on every workgroup of a launch
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device_id) == hipSuccess) {
        limits.n_cus = std::max(1, prop.multiProcessorCount);
        limits.lds_per_cu = (int)std::max<size_t>(prop.maxSharedMemoryPerMultiProcessor, prop.sharedMemPerBlock);
    }
    EnginePlan plan;
    if (const int rc = plan_engine(c, ext, limits, create_knobs(), &plan, &why)) return fail(rc, "%s", why.c_str());

    frl_engine* e = new frl_engine();      // (nothing is refused from here on: CREATE_TRY undoes what a failed HIP call leaves)
    e->cfg = c;
    e->h = plan.h;
    static_cast<EngineFacts&>(*e) = plan;
    EngineDesc& h = e->h;
    const RecordDesc& R = h.rec;
    const AlgoTraits& T = algo_traits(c.algo);

#define CREATE_TRY(expr)                                                                           \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            int rc_ = fail(FRL_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));                   \
            frl_destroy(e);                                                                        \
            return rc_;                                                                            \
        }                                                                                          \
    } while (0)

    CREATE_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    CREATE_TRY(hipEventCreate(&e->ev0));
    CREATE_TRY(hipEventCreate(&e->ev1));
    CREATE_TRY(hipEventCreateWithFlags(&e->ev_stage, hipEventDisableTiming));
    const size_t P = h.P;
    CREATE_TRY(e->mem.alloc_zero(&h.replay, P * (size_t)h.capacity * R.stride, e->stream));
    if (e->has_nets) {
        const size_t ls = h.learner_stride;
        CREATE_TRY(e->mem.alloc_zero(&h.theta, P * ls, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.target, P * ls, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.m, P * ls, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.v, P * ls, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.grad, P * ls, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.slab, e->slab_count, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.part, e->part_count, e->stream));
        if (e->act_spill_count) CREATE_TRY(e->mem.alloc_zero(&h.act_spill, e->act_spill_count, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.gsq, P * (size_t)h.n_agents * h.Gmax, e->stream));
        if (h.noisy) {
            CREATE_TRY(e->mem.alloc_zero(&h.theta_eff, P * 3 * ls, e->stream));
            CREATE_TRY(e->mem.alloc_zero(&h.noisy_eps, P * 3 * (size_t)e->noisy_per_set, e->stream));
            CREATE_TRY(e->mem.alloc(&e->h_noisy, P * 3 * (size_t)e->noisy_per_set, MEM_PINNED));
        }
        CREATE_TRY(e->mem.alloc_zero(&h.isw, P * (size_t)h.batch_max, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.td_err, P * (size_t)h.batch_max, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.idx, e->idx_count, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.noise, e->noise_count, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.stats, P * h.n_agents * ST_COUNT, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.steps, e->steps_count, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.ticket, P + 1, e->stream));
        CREATE_TRY(e->mem.alloc_zero(&h.alpha, e->alpha_count, e->stream));
        if (c.algo == FRL_ALGO_REINFORCE) {
            CREATE_TRY(e->mem.alloc_zero(&h.ep_n, P, e->stream));
            CREATE_TRY(e->mem.alloc(&e->h_ep_n, 2 * P, MEM_PINNED));
            for (hipEvent_t& ev : e->ev_ep) CREATE_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
        if (c.algo == FRL_ALGO_CEM_GD3PG) {
            CREATE_TRY(e->mem.alloc_zero(&h.cem_ctl, 2 * P, e->stream));
            CREATE_TRY(e->mem.alloc_zero(&h.cem_out, 8 * P, e->stream));
            CREATE_TRY(e->mem.alloc(&e->h_cem_ctl, 4 * P, MEM_PINNED));
            for (hipEvent_t& ev : e->ev_ep) CREATE_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
        if (c.algo == FRL_ALGO_GAIL) {
            const size_t rows_n = P * (size_t)h.batch_max * (c.obs_dim[0] + c.act_dim[0]);
            CREATE_TRY(e->mem.alloc_zero(&h.gail_rows, rows_n, e->stream));
            CREATE_TRY(e->mem.alloc_zero(&h.gail_part, P * (size_t)h.S * 8, e->stream));
            CREATE_TRY(e->mem.alloc_zero(&h.gail_out, P * 8, e->stream));
            CREATE_TRY(e->mem.alloc(&e->h_gail_rows, rows_n, MEM_PINNED));
        }
        if (T.vector_reward) {
            CREATE_TRY(e->mem.alloc_zero(&h.env_w, P * (size_t)h.batch_max * h.reward_dim, e->stream));
            CREATE_TRY(e->mem.alloc(&e->h_env_w, P * (size_t)h.batch_max * h.reward_dim, MEM_PINNED));
        }
        if (h.solo || h.solow) {
            const size_t U = P * (size_t)h.n_agents, NT = h.solow ? (size_t)h.solow : (size_t)kSoloWG;      // (kernels_solow.hip: units, row tiles per unit)
            CREATE_TRY(e->mem.alloc_zero(&e->d_solo_slab, U * NT * e->solo_stride, e->stream));
            CREATE_TRY(e->mem.alloc_zero(&e->d_solo_part, U * (size_t)std::max((int)NT, e->solow_wgs) * kSoloPartHost, e->stream));
            CREATE_TRY(e->mem.alloc_zero(&e->d_solo_pre, 2 * U * (size_t)std::max(kSoloPre, 8 + h.batch_max), e->stream));
            CREATE_TRY(e->mem.alloc_zero(&e->d_solo_bar, 2 * U * NT + 2, e->stream));      // [units][tiles] slab flags, then as many "actor slice stepped" flags (kernels_solo.hip: offset P * 16),
            e->d_solo_ticket = (int*)(e->d_solo_bar + 2 * U * NT);                         // ... and, in the same block, the rollout tail's learner ticket
            if (h.solow) CREATE_TRY(e->mem.alloc_zero(&e->d_solow_bar2, U * 64, e->stream));
        }
        if (h.solo || h.solow || h.algo == ALGO_DQN) {                     // the pinned give-up word of the spinning launches (solo hand-overs, pre-armed DQN steps)
            CREATE_TRY(e->mem.alloc(&e->h_solo_err, 64 / sizeof(int), MEM_PINNED, hipHostMallocCoherent | hipHostMallocMapped));
            *e->h_solo_err = 0;
            CREATE_TRY(hipHostGetDevicePointer((void**)&e->d_solo_err, e->h_solo_err, 0));
        }
        if (e->actor_park_count) CREATE_TRY(e->mem.alloc_zero(&h.actor_park, e->actor_park_count, e->stream));
        if (h.wide) CREATE_TRY(e->mem.alloc_zero(&h.wide_scr, P * (size_t)h.n_agents * h.wide_unit, e->stream));
        if (h.wide || h.solow) {                                           // select_action's Wk-layout copies of the nets (launch_act)
            e->act_wk_version.assign(2 * (size_t)h.n_nets, 0ULL);
            CREATE_TRY(e->mem.alloc(&e->d_act_wk, 2 * (size_t)h.n_nets * e->act_wk_slot, MEM_DEVICE));
        }
        CREATE_TRY(e->mem.alloc_zero(&h.obsnorm, P * (size_t)c.n_agents * c.n_agents * h.obsnorm_w, e->stream));
        CREATE_TRY(e->mem.alloc(&e->h_idx, e->idx_count, MEM_PINNED));
        CREATE_TRY(e->mem.alloc(&e->h_noise, e->noise_count, MEM_PINNED));
    }
    e->stage_cap = 4096;
    CREATE_TRY(e->mem.alloc(&e->stage_rows, (size_t)e->stage_cap * R.width, MEM_PINNED));
    CREATE_TRY(e->mem.alloc(&e->stage_slots, (size_t)e->stage_cap, MEM_PINNED));
    CREATE_TRY(e->mem.alloc(&e->d_stage_rows, (size_t)e->stage_cap * R.width, MEM_DEVICE));
    CREATE_TRY(e->mem.alloc(&e->d_stage_slots, (size_t)e->stage_cap, MEM_DEVICE));
    CREATE_TRY(e->mem.alloc(&e->h_idx64, (size_t)h.batch_max * 16, MEM_PINNED));
    CREATE_TRY(e->mem.alloc(&e->d_idx64, (size_t)h.batch_max * 16, MEM_DEVICE));
    CREATE_TRY(e->mem.alloc(&e->d, 1, MEM_DEVICE));
    CREATE_TRY(hipMemcpyAsync(e->d, &h, sizeof h, hipMemcpyHostToDevice, e->stream));
    e->index.assign(P * e->n_rings, 0);
    e->size.assign(P * e->n_rings, 0);
    e->staged_per_learner.assign(P, 0);
    if (h.algo == ALGO_DQN) CREATE_TRY(set_family_lds_attributes(FAM_DQN_FUSED));
    if (h.algo == ALGO_DQN || e->family != FAM_ROWCHUNK) e->kern = resolve_learn_kernels(h.algo == ALGO_DQN ? FAM_DQN_FUSED : e->family, e->chain_waves, e->actor_park, h);
    // (a vector reward: batch_max counts rows = batch x weight_num; the draw is for `batch` of them)
    if (h.batch_max > 256 && (4 * h.batch_max <= kDrawTableHost || T.vector_reward))     // draw_kernel's duplicate table for batches of 257 .. 2048 rows (device/net.hpp)
        CREATE_TRY(hipFuncSetAttribute((const void*)draw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (2 * 2048 + 2 * kDrawTableHost) * (int)sizeof(int)));
    if (e->family != FAM_ROWCHUNK) CREATE_TRY(set_family_lds_attributes(e->family));
    if (e->family == FAM_SOLO || e->family == FAM_CHAINED)         // select_action on fragment-image nets, the solo rollout tail's act_frag_body
        CREATE_TRY(hipFuncSetAttribute((const void*)act_frag_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, critic2_lds_floats() * (int)sizeof(float)));
    if (e->lds_bytes > 64 * 1024) {
        for (const void* k : {(const void*)dqn_grad_kernel, (const void*)ac_critic_kernel, (const void*)ac_actor_kernel, (const void*)sacd_critic_kernel, (const void*)sacd_actor_kernel,
                              (const void*)reinforce_grad_kernel, (const void*)envelope_grad_kernel, (const void*)envelope_ddpg_critic_kernel,
                              (const void*)envelope_ddpg_actor_kernel, (const void*)gail_disc_kernel, (const void*)gail_forward_kernel, (const void*)act_kernel,
                              (const void*)ppo_update_kernel, (const void*)mappo_values_kernel, (const void*)mappo_update_kernel, (const void*)mappo_act_kernel,
                              (const void*)happo_update_kernel, (const void*)mappo_mask_update_kernel, (const void*)mappo_mask_act_kernel,
                              (const void*)mappo_state_values_kernel, (const void*)mappo_state_update_kernel, (const void*)mappo_state_mask_update_kernel,
                              (const void*)att_q_kernel, (const void*)masac_act_kernel, (const void*)gail_ppo_prepare_kernel,
                              (const void*)gail_ppo_update_kernel, (const void*)gail_ppo_act_kernel, (const void*)cem_critic_kernel, (const void*)cem_actor_kernel,
                              (const void*)cem_act_kernel})
            CREATE_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes));
        if (h.algo == ALGO_DDPG || h.algo == ALGO_TD3 || h.algo == ALGO_SAC) CREATE_TRY(set_family_lds_attributes(FAM_CHAINED));
        if (h.algo == ALGO_PPO)
            for (auto k : {ppo_update_v2_k1_relu, ppo_update_v2_k2_relu, ppo_update_v2_k1_tanh, ppo_update_v2_k2_tanh})
                CREATE_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, ppo2_lds_floats(2) * (int)sizeof(float)));
    }
    CREATE_TRY(hipStreamSynchronize(e->stream));
    *out = e;
    return FRL_OK;
}

#define ENG(e)                                                  \
    if (!(e)) return fail(FRL_ERR_INVALID, "engine is NULL");   \
    HIP_TRY(hipSetDevice((e)->cfg.device_id))

// kernels_solo.hip's hand-overs spin on flags of the learner's other workgroups, which therefore must all be resident; a workgroup that
// has waited 2 s gives up, sets the pinned word and the launch's numbers are not valid.  That takes something else holding this GPU's CUs
// for seconds (another process' long kernel): reported at the next synchronising call instead of passing silently.
static int solo_err_check(frl_engine* e) {
    if (!e->h_solo_err || *(volatile int*)e->h_solo_err == 0) return FRL_OK;
    const int what = *(volatile int*)e->h_solo_err;
    *(volatile int*)e->h_solo_err = 0;
    if (what == 2)
        return fail(FRL_ERR_STATE, "dqn_fused_kernel: a pre-armed rollout launch waited 2 s for the previous launch or for the host's doorbell and gave up; "
                                   "its update and the actions it was to select were dropped");
    return fail(FRL_ERR_STATE, "kernels_solo.hip / kernels_solow.hip: a workgroup waited 2 s for the other workgroups of its learner (is something else holding this GPU's "
                               "CUs?); the updates since the last synchronising call are not valid");
}

extern "C" int frl_sync(frl_engine* e) {
    ENG(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    return solo_err_check(e);
}

extern "C" int frl_lds_bytes(const frl_engine* e, int* bytes_out, int* rc_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    if (bytes_out) *bytes_out = e->lds_bytes;
    if (rc_out) *rc_out = e->h.rc;
    return FRL_OK;
}

extern "C" int frl_state_info(const frl_engine* e, int* state_dim_out, int* state_col_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    if (state_dim_out) *state_dim_out = e->h.state_dim;
    if (state_col_out) *state_col_out = e->h.state_off;
    return FRL_OK;
}

// ----------------------------------------------------------------------------------- replay
extern "C" int frl_record_layout_get(const frl_engine* e, frl_record_layout* out) {
    if (!e || !out) return fail(FRL_ERR_INVALID, "NULL argument");
    record_layout(e->h.rec, out);
    return FRL_OK;
}

static int flush_stage(frl_engine* e) {
    if (e->stage_n == 0) return FRL_OK;
    const RecordDesc& R = e->h.rec;
    const int n = e->stage_n;
    HIP_TRY(hipMemcpyAsync(e->d_stage_rows, e->stage_rows, (size_t)n * R.width * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_stage_slots, e->stage_slots, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, e->stream));
    const int per_row = (R.width + 3) / 4;
    const long long total = (long long)n * per_row;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(replay_scatter_kernel, dim3(blocks), dim3(256), 0, e->stream, e->h.replay, e->d_stage_rows,
                       e->d_stage_slots, n, R.width, R.stride);
    HIP_TRY(hipGetLastError());
    if (e->per_on) {                 // PER_Buffer.add (Buffer.py:92-98): the new rows enter at the current maximum priority
        // bucket the flush's rows by learner (counting sort; rows keep their staging order inside a bucket)
        const int P = e->h.P, cap = e->h.capacity;
        int* off = e->stage_bucket;
        int* before = off + P + 1;
        int* leaf = before + P;
        std::fill(off, off + P + 1, 0);
        for (int i = 0; i < n; ++i) off[e->stage_slots[i] / cap + 1]++;
        for (int p = 0; p < P; ++p) off[p + 1] += off[p];
        std::vector<int>& cur = e->bucket_cursor;
        cur.assign(off, off + P);
        for (int i = 0; i < n; ++i) { const long long s = e->stage_slots[i]; const int p = (int)(s / cap); leaf[cur[p]++] = (int)(s - (long long)p * cap); }
        memcpy(before, e->size_flushed.data(), (size_t)P * sizeof(int));
        HIP_TRY(hipMemcpyAsync(e->d_stage_bucket, e->stage_bucket, (size_t)(2 * P + 1 + n) * sizeof(int), hipMemcpyHostToDevice, e->stream));
        PerArgs pa;
        memset(&pa, 0, sizeof pa);
        pa.sum_tree = e->d_per_sum; pa.max_tree = e->d_per_max; pa.cap = cap; pa.n = n;
        hipLaunchKernelGGL(per_add_kernel, dim3(P), dim3(256), 0, e->stream, pa, (const int*)e->d_stage_bucket, P);
        HIP_TRY(hipGetLastError());
    }
    e->size_flushed = e->size;
    HIP_TRY(hipEventRecord(e->ev_stage, e->stream));
    e->stage_inflight = true;
    e->stage_n = 0;
    std::fill(e->staged_per_learner.begin(), e->staged_per_learner.end(), 0);
    return FRL_OK;
}

// ring: which of the learner's rings (0 everywhere but on a CEM_GD3PG engine; ring r's rows are the learner's rows [r ring_cap, (r + 1) ring_cap))
static int stage_one(frl_engine* e, int learner, const float* record, int ring = 0) {
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner %d out of range", learner);
    if (ring < 0 || ring >= e->n_rings) return fail(FRL_ERR_INVALID, "ring %d out of range (the engine has %d per learner)", ring, e->n_rings);
    // one scatter launch writes its rows in no particular order: never stage the same ring row twice
    if (e->stage_n == e->stage_cap || e->staged_per_learner[learner] >= e->ring_cap) { int rc = flush_stage(e); if (rc) return rc; }
    if (e->stage_inflight) {     // the pinned area may still be read by the previous flush's copy
        HIP_TRY(hipEventSynchronize(e->ev_stage));
        e->stage_inflight = false;
    }
    const RecordDesc& R = e->h.rec;
    memcpy(e->stage_rows + (size_t)e->stage_n * R.width, record, (size_t)R.width * sizeof(float));
    const size_t cur = (size_t)ring * e->h.P + learner;
    int& ix = e->index[cur];
    e->stage_slots[e->stage_n] = (long long)learner * e->h.capacity + (long long)ring * e->ring_cap + ix;
    e->stage_n++;
    e->staged_per_learner[learner]++;
    ix = (ix + 1) % e->ring_cap;                          // Buffer.py:36
    if (e->size[cur] < e->ring_cap) e->size[cur]++;       // Buffer.py:37-38
    return FRL_OK;
}

extern "C" int frl_buffer_add(frl_engine* e, int learner, const float* record) {
    ENG(e);
    if (!record) return fail(FRL_ERR_INVALID, "record is NULL");
    return stage_one(e, learner, record);
}

extern "C" int frl_buffer_add_batch(frl_engine* e, int n, const int* learners, const float* records) {
    ENG(e);
    if (n < 0 || (n > 0 && !records)) return fail(FRL_ERR_INVALID, "bad batch");
    const int w = e->h.rec.width;
    for (int i = 0; i < n; ++i) {
        int rc = stage_one(e, learners ? learners[i] : 0, records + (size_t)i * w);
        if (rc) return rc;
    }
    return FRL_OK;
}

extern "C" int frl_buffer_flush(frl_engine* e) {
    ENG(e);
    return flush_stage(e);
}

extern "C" int frl_buffer_cursor_get(const frl_engine* e, int learner, int* index_out, int* size_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner out of range");
    if (index_out) *index_out = e->index[learner];
    if (size_out) *size_out = e->size[learner];
    return FRL_OK;
}

extern "C" int frl_buffer_cursor_set(frl_engine* e, int learner, int index, int size) {
    ENG(e);
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner out of range");
    if (index < 0 || index >= e->ring_cap || size < 0 || size > e->ring_cap)
        return fail(FRL_ERR_INVALID, "cursor (%d,%d) outside capacity %d", index, size, e->ring_cap);
    // rows staged before the cursor moves are committed first: afterwards the same ring slot may be staged again, and one
    // scatter launch must never hold a slot twice (it writes its rows in no particular order)
    int rc = flush_stage(e);
    if (rc) return rc;
    e->index[learner] = index;
    e->size[learner] = size;
    return FRL_OK;
}

extern "C" int frl_buffer_sample(frl_engine* e, int learner, const int64_t* idx, int batch, int n_fields,
                                 const int* col0, const int* ncols, float* const* out_device) {
    ENG(e);
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner out of range");
    if (batch < 0 || batch > e->h.batch_max * 16) return fail(FRL_ERR_INVALID, "batch %d exceeds 16*batch_max", batch);
    if (n_fields < 1 || n_fields > 8 || !idx || !col0 || !ncols || !out_device) return fail(FRL_ERR_INVALID, "bad field list");
    if (batch == 0) return FRL_OK;
    const RecordDesc& R = e->h.rec;
    GatherFields F;
    memset(&F, 0, sizeof F);
    F.n_fields = n_fields;
    for (int f = 0; f < n_fields; ++f) {
        if (col0[f] < 0 || ncols[f] < 1 || col0[f] + ncols[f] > R.width) return fail(FRL_ERR_INVALID, "field %d outside the record", f);
        F.col0[f] = col0[f]; F.ncols[f] = ncols[f]; F.out[f] = out_device[f];
    }
    for (int i = 0; i < batch; ++i)     // NumPy fancy indexing semantics: negative wraps, out of range raises
        if (idx[i] < -(int64_t)e->h.capacity || idx[i] >= e->h.capacity) return fail(FRL_ERR_INVALID, "index %lld out of range", (long long)idx[i]);
    int rc = flush_stage(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));            // h_idx64 reuse
    for (int i = 0; i < batch; ++i) e->h_idx64[i] = idx[i] < 0 ? idx[i] + e->h.capacity : idx[i];
    HIP_TRY(hipMemcpyAsync(e->d_idx64, e->h_idx64, (size_t)batch * sizeof(long long), hipMemcpyHostToDevice, e->stream));
    const float* ring = e->h.replay + (size_t)learner * e->h.capacity * R.stride;
    const int threads = 256, groups_per_block = threads / 16;
    hipLaunchKernelGGL(replay_gather_kernel, dim3((batch + groups_per_block - 1) / groups_per_block), dim3(threads), 0,
                       e->stream, ring, e->d_idx64, batch, R.stride, F);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));            // outputs are consumed on the caller's stream
    return FRL_OK;
}

extern "C" int frl_buffer_read(frl_engine* e, int learner, int row0, int n, float* out_host) {
    ENG(e);
    if (learner < 0 || learner >= e->h.P || row0 < 0 || n < 0 || row0 + n > e->h.capacity || !out_host)
        return fail(FRL_ERR_INVALID, "bad read range");
    if (n == 0) return FRL_OK;
    int rc = flush_stage(e);
    if (rc) return rc;
    const RecordDesc& R = e->h.rec;
    float* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&tmp, (size_t)n * R.width * sizeof(float)));
    const long long total = (long long)n * R.width;
    hipLaunchKernelGGL(replay_read_kernel, dim3((int)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0, e->stream,
                       e->h.replay, (long long)learner * e->h.capacity + row0, n, R.width, R.stride, tmp);
    hipError_t err = hipMemcpyAsync(out_host, tmp, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    hipFree(tmp);
    if (err != hipSuccess) return fail(FRL_ERR_HIP, "frl_buffer_read: %s", hipGetErrorString(err));
    return FRL_OK;
}

extern "C" int frl_buffer_fill_synthetic(frl_engine* e, int rows, uint64_t seed) {
    ENG(e);
    if (rows < 0 || rows > e->ring_cap) return fail(FRL_ERR_INVALID, "rows out of range");
    if (e->per_on)       // priorities are assigned by add (PER_Buffer.add, Buffer.py:92-98): a bulk fill would leave the trees empty
        return fail(FRL_ERR_STATE, "frl_buffer_fill_synthetic bypasses the priority trees: fill a PER engine through frl_buffer_add_batch");
    int rc = flush_stage(e);
    if (rc) return rc;
    const RecordDesc& R = e->h.rec;
    for (int p = 0; p < e->h.P; ++p) {
        float* ring = e->h.replay + (size_t)p * e->h.capacity * R.stride;
        hipLaunchKernelGGL(replay_fill_kernel, dim3(std::min((rows + 255) / 256, 2048)), dim3(256), 0, e->stream, ring,
                           (long long)rows, R, e->h.n_discrete, seed + 0x632BE59BD9B4E019ull * (p + 1));
        e->index[p] = rows % e->ring_cap;
        e->size[p] = rows;
    }
    HIP_TRY(hipGetLastError());
    return FRL_OK;
}

// ------------------------------------------------------------------------------- parameters
extern "C" int frl_net_count(const frl_engine* e, int* n_out) {
    if (!e || !n_out) return fail(FRL_ERR_INVALID, "NULL argument");
    *n_out = e->h.n_nets;
    return FRL_OK;
}

extern "C" int frl_net_num_params(const frl_engine* e, int net, int* n_out) {
    if (!e || !n_out) return fail(FRL_ERR_INVALID, "NULL argument");
    if (net < 0 || net >= e->h.n_nets) return fail(FRL_ERR_INVALID, "net %d out of range", net);
    *n_out = e->h.net[net].n_params;
    return FRL_OK;
}

static float* kind_ptr(frl_engine* e, int kind) {
    switch (kind) {
        case FRL_PARAM_ONLINE: return e->h.theta;
        case FRL_PARAM_TARGET: return e->h.target;
        case FRL_PARAM_ADAM_M: return e->h.m;
        case FRL_PARAM_ADAM_V: return e->h.v;
        case FRL_PARAM_GRAD: return e->h.grad;
    }
    return nullptr;
}

static int params_xfer(frl_engine* e, int learner, int net, int kind, float* host, bool to_device) {
    ENG(e);
    if (!e->has_nets) return fail(FRL_ERR_STATE, "replay-only engine has no networks");
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner out of range");
    if (net < 0 || net >= e->h.n_nets) return fail(FRL_ERR_INVALID, "net %d out of range", net);
    float* base = kind_ptr(e, kind);
    if (!base || !host) return fail(FRL_ERR_INVALID, "bad kind / NULL buffer");
    const NetDesc& N = e->h.net[net];
    float* dev = base + (size_t)learner * e->h.learner_stride + e->h.net_off[net];
    // host order = the reference's state_dict order: per nn.Linear weight[out][in] then bias; device block =
    // Wk[k_pad][n_pad], or the fragment-image order of the register-chained engines (frl_desc.h: weight_index)
    std::vector<float> blk(N.size, 0.f);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (!to_device) {
        const int rs = solo_err_check(e);
        if (rs) return rs;
        HIP_TRY(hipMemcpy(blk.data(), dev, (size_t)N.size * sizeof(float), hipMemcpyDeviceToHost));
    }
    size_t o = 0;
    for (int i = 0; i < N.n_layers + N.n_shadow; ++i) {       // shadow layers (a noisy head's sigma) follow the forward ones
        const LayerDesc& L = N.L[i];
        // (a MASAC actor's head is mean_layer and log_std_layer stacked: the host order is each nn.Linear's weight then bias, MASAC.py:37-38)
        const int parts = (e->h.algo == ALGO_MASAC && !(net & 1) && i == N.n_layers - 1) ? 2 : 1, rows = L.n / parts;
        for (int part = 0; part < parts; ++part) {
            for (int r = part * rows; r < (part + 1) * rows; ++r)
                for (int c = 0; c < L.k; ++c) {
                    float& d = blk[L.w_off + weight_index(N, L, r, c)];
                    if (to_device) d = host[o]; else host[o] = d;
                    ++o;
                }
            for (int r = part * rows; r < (part + 1) * rows; ++r) {
                float& d = blk[L.b_off + r];
                if (to_device) d = host[o]; else host[o] = d;
                ++o;
            }
        }
    }
    for (int j = 0; j < N.extra_n; ++j) {
        float& d = blk[N.extra_off + j];
        if (to_device) d = host[o]; else host[o] = d;
        ++o;
    }
    if (to_device) {
        HIP_TRY(hipMemcpy(dev, blk.data(), (size_t)N.size * sizeof(float), hipMemcpyHostToDevice));
        ++e->param_version;
    }
    return FRL_OK;
}

extern "C" int frl_params_get(frl_engine* e, int learner, int net, int kind, float* out_host) {
    return params_xfer(e, learner, net, kind, out_host, false);
}
extern "C" int frl_params_set(frl_engine* e, int learner, int net, int kind, const float* in_host) {
    return params_xfer(e, learner, net, kind, const_cast<float*>(in_host), true);
}

extern "C" int frl_params_pad_max(frl_engine* e, int learner, int net, int kind, float* max_abs_out) {
    ENG(e);
    if (!e->has_nets) return fail(FRL_ERR_STATE, "replay-only engine has no networks");
    if (learner < 0 || learner >= e->h.P || net < 0 || net >= e->h.n_nets || !max_abs_out) return fail(FRL_ERR_INVALID, "bad argument");
    float* base = kind_ptr(e, kind);
    if (!base) return fail(FRL_ERR_INVALID, "bad kind");
    const NetDesc& N = e->h.net[net];
    std::vector<float> blk(N.size, 0.f);
    std::vector<char> real(N.size, 0);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(blk.data(), base + (size_t)learner * e->h.learner_stride + e->h.net_off[net], (size_t)N.size * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < N.n_layers + N.n_shadow; ++i) {
        const LayerDesc& L = N.L[i];
        for (int r = 0; r < L.n; ++r) {
            for (int c = 0; c < L.k; ++c) real[L.w_off + weight_index(N, L, r, c)] = 1;
            real[L.b_off + r] = 1;
        }
    }
    for (int j = 0; j < N.extra_n; ++j) real[N.extra_off + j] = 1;
    float mx = 0.f;
    for (int i = 0; i < N.size; ++i)
        if (!real[i]) mx = std::max(mx, std::isnan(blk[i]) ? INFINITY : std::fabs(blk[i]));
    *max_abs_out = mx;
    return FRL_OK;
}

extern "C" int frl_opt_step_get(frl_engine* e, int learner, int net, int* t_out) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || net < 0 || net > kMaxNets || !t_out) return fail(FRL_ERR_INVALID, "bad argument");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(t_out, e->h.steps + (size_t)learner * (kMaxNets + 1) + net, sizeof(int), hipMemcpyDeviceToHost));
    return FRL_OK;
}
extern "C" int frl_opt_step_set(frl_engine* e, int learner, int net, int t) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || net < 0 || net > kMaxNets) return fail(FRL_ERR_INVALID, "bad argument");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->h.steps + (size_t)learner * (kMaxNets + 1) + net, &t, sizeof(int), hipMemcpyHostToDevice));
    return FRL_OK;
}

// MASAC: one alpha block per (learner, agent), the agents' step counts behind the nets' (frl_desc.h: EngineDesc::alpha, ::steps)
static int masac_alpha_xfer(frl_engine* e, int learner, int agent, float* vals4, int* step, bool to_device) {
    const EngineDesc& h = e->h;
    float* al = h.alpha + ((size_t)learner * h.n_agents + agent) * 4;
    int* cnt = h.steps + (size_t)h.P * (kMaxNets + 1) + (size_t)learner * h.n_agents + agent;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(to_device ? (void*)al : (void*)vals4, to_device ? (const void*)vals4 : (const void*)al, 4 * sizeof(float), to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    if (step) HIP_TRY(hipMemcpy(to_device ? (void*)cnt : (void*)step, to_device ? (const void*)step : (const void*)cnt, sizeof(int), to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return FRL_OK;
}
extern "C" int frl_alpha_get_agent(frl_engine* e, int learner, int agent, float* vals4_out, int* step_out) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || agent < 0 || agent >= e->h.n_agents || !vals4_out) return fail(FRL_ERR_INVALID, "bad argument");
    if (e->h.algo != ALGO_MASAC) return agent == 0 ? frl_alpha_get(e, learner, vals4_out, step_out) : fail(FRL_ERR_INVALID, "agent %d: a %s engine has one alpha per learner", agent, algo_traits(e->h.algo).name);
    return masac_alpha_xfer(e, learner, agent, vals4_out, step_out, false);
}
extern "C" int frl_alpha_set_agent(frl_engine* e, int learner, int agent, const float* vals4, int step) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || agent < 0 || agent >= e->h.n_agents || !vals4) return fail(FRL_ERR_INVALID, "bad argument");
    if (e->h.algo != ALGO_MASAC) return agent == 0 ? frl_alpha_set(e, learner, vals4, step) : fail(FRL_ERR_INVALID, "agent %d: a %s engine has one alpha per learner", agent, algo_traits(e->h.algo).name);
    return masac_alpha_xfer(e, learner, agent, const_cast<float*>(vals4), &step, true);
}

extern "C" int frl_alpha_get(frl_engine* e, int learner, float* vals4_out, int* step_out) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || !vals4_out) return fail(FRL_ERR_INVALID, "bad argument");
    if (e->h.algo == ALGO_MASAC)
        return e->h.n_agents > 1 ? fail(FRL_ERR_STATE, "frl_alpha_get: a MASAC engine has one alpha per agent: frl_alpha_get_agent") : masac_alpha_xfer(e, learner, 0, vals4_out, step_out, false);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(vals4_out, e->h.alpha + (size_t)learner * 4, 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (step_out) return frl_opt_step_get(e, learner, kMaxNets, step_out);
    return FRL_OK;
}
extern "C" int frl_alpha_set(frl_engine* e, int learner, const float* vals4, int step) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || !vals4) return fail(FRL_ERR_INVALID, "bad argument");
    if (e->h.algo == ALGO_MASAC)
        return e->h.n_agents > 1 ? fail(FRL_ERR_STATE, "frl_alpha_set: a MASAC engine has one alpha per agent: frl_alpha_set_agent") : masac_alpha_xfer(e, learner, 0, const_cast<float*>(vals4), &step, true);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->h.alpha + (size_t)learner * 4, vals4, 4 * sizeof(float), hipMemcpyHostToDevice));
    return frl_opt_step_set(e, learner, kMaxNets, step);
}

// -------------------------------------------------------------------------------------- act
// Exploration folded into an act launch (ActArgs' second half): the device pointers a collector owns.
struct ActExplore {
    frl_explore_args x;
    const float* scale_dev = nullptr;          // [P] or nullptr (x.scale for everybody)
    float* ou_state_dev = nullptr;             // [P][n_rows][A]
    const unsigned char* flags_dev = nullptr;  // [P][n_rows]
    float* env_out_dev = nullptr;              // [P][n_rows][A] (discrete: [P][n_rows])
    bool device_eps = false;
};

// build_only: fill *build_only with the launch's arguments and return without launching or consuming a Philox counter (the caller
// sets rng_counter: frl_rollout's folded step, whose act rides on the learn launches)
static int launch_act(frl_engine* e, int net, int mode_flags, int head, int use_target, int n_rows, int in_dim,
                      const float* in_dev, const float* eps_dev, float* out_dev, float* logp_dev, const ActExplore* ex = nullptr,
                      ActArgs* build_only = nullptr) {
    int mode = mode_flags & ~FRL_ACT_NO_OBSNORM;
    if (!e->has_nets) return fail(FRL_ERR_STATE, "replay-only engine has no networks");
    if (net < 0 || net >= e->h.n_nets) return fail(FRL_ERR_INVALID, "net %d out of range", net);
    const NetDesc& N = e->h.net[net];
    if (head < 0 || head >= N.heads) return fail(FRL_ERR_INVALID, "head out of range");
    const int nl = N.n_layers / N.heads;
    // (an attention critic's rows are [all obs | all actions]: x_e and x_d are cut from them in the kernel)
    const int want_in = (e->h.algo == ALGO_MADDPG_ATT && (net & 1)) ? e->h.rec.obs_total + e->h.rec.act_total : N.L[head * nl].k;
    if (in_dim != want_in) return fail(FRL_ERR_INVALID, "in_dim %d != layer input %d", in_dim, want_in);
    const bool masac_actor = e->h.algo == ALGO_MASAC && !(net & 1);      // its log_std is the head's second half, not an extra vector
    if ((mode == FRL_ACT_SAC_SAMPLE || mode == FRL_ACT_PPO_SAMPLE) && N.extra_n == 0 && !(masac_actor && mode == FRL_ACT_SAC_SAMPLE)) return fail(FRL_ERR_INVALID, "net has no log_std");
    const bool gail_ppo = e->h.algo == ALGO_GAIL_PPO;      // (its sampling modes draw for themselves when no eps is given: below)
    if (mode == FRL_ACT_CAT_SAMPLE && !eps_dev && !(ex && ex->device_eps) && !gail_ppo) return fail(FRL_ERR_INVALID, "FRL_ACT_CAT_SAMPLE needs the Exp(1) draws in eps");
    if (n_rows < 1) return fail(FRL_ERR_INVALID, "n_rows must be >= 1");
    const bool no_norm = (mode_flags & FRL_ACT_NO_OBSNORM) != 0;
    ActArgs a;
    memset(&a, 0, sizeof a);
    if (ex) {
        frl_explore_args x = ex->x;
        if (x.kind == FRL_EXPLORE_OFF) return fail(FRL_ERR_INVALID, "FRL_EXPLORE_OFF is a frl_rollout_args value; frl_explore_args.kind takes FRL_EXPLORE_NONE");
        if (x.kind < FRL_EXPLORE_NONE || x.kind > FRL_EXPLORE_OU) return fail(FRL_ERR_INVALID, "unknown exploration kind %d", x.kind);
        if (!ex->env_out_dev) return fail(FRL_ERR_INVALID, "exploration needs an env-action output");
        if (x.kind == FRL_EXPLORE_EPS_GREEDY && mode != FRL_ACT_ARGMAX) return fail(FRL_ERR_INVALID, "epsilon-greedy goes with FRL_ACT_ARGMAX");
        if ((x.kind == FRL_EXPLORE_GAUSS || x.kind == FRL_EXPLORE_OU) && !(mode == FRL_ACT_TANHHEAD || mode == FRL_ACT_SAC_SAMPLE))
            return fail(FRL_ERR_INVALID, "Gaussian / OU action noise goes with FRL_ACT_TANHHEAD or FRL_ACT_SAC_SAMPLE");
        if (x.kind == FRL_EXPLORE_OU && !ex->ou_state_dev) return fail(FRL_ERR_INVALID, "OU exploration needs a state buffer");
        a.explore = x.kind; a.device_eps = ex->device_eps ? 1 : 0;
        a.epsilon = x.epsilon; a.sigma = x.sigma; a.scale0 = x.scale; a.max_action = x.max_action != 0.f ? x.max_action : 1.f;
        a.ou_theta = x.ou_theta; a.ou_sigma = x.ou_sigma; a.ou_dt = x.ou_dt;
        a.scale = ex->scale_dev; a.ou_state = ex->ou_state_dev; a.flags = ex->flags_dev; a.env_out = ex->env_out_dev;
        if (!build_only) a.rng_counter = e->rng_counter++;
    }
    a.net = net; a.use_target = use_target; a.mode = mode; a.n_rows = n_rows; a.head = head; a.in_dim = in_dim;
    const int agent = e->h.n_agents > 1 ? net / 2 : 0;            // MADDPG: only the actors (even nets) take a single agent's obs
    a.normalize = (!no_norm && e->h.obs_norm_on && (e->h.n_agents == 1 || net % 2 == 0) && in_dim == e->h.rec.obs_dim[agent]) ? 1 : 0;
    a.in = in_dev; a.eps = eps_dev; a.out = out_dev; a.out_logp = logp_dev;
    if (build_only) { *build_only = a; return FRL_OK; }
    if (is_mappo_family(e->h.algo)) {        // the normalised forward (kernels_mappo.hip) in front of act_kernel's epilogue
        if (mode == FRL_ACT_SAC_SAMPLE || ex) return fail(FRL_ERR_INVALID, "a %s engine acts through FRL_ACT_RAW, _TANHHEAD, _ARGMAX, _PPO_SAMPLE or _CAT_SAMPLE", algo_traits(e->h.algo).name);
        hipLaunchKernelGGL(mappo_act_kernel, dim3((n_rows + e->h.rc - 1) / e->h.rc, e->h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
        HIP_TRY(hipGetLastError());
        return FRL_OK;
    }
    if (e->h.algo == ALGO_MADDPG_ATT && (net & 1)) {      // the attention critic is no chain: its own forward (kernels_att.hip), Q of [all obs | all actions]
        if (mode != FRL_ACT_RAW || ex) return fail(FRL_ERR_INVALID, "an ATT-MADDPG critic acts through FRL_ACT_RAW on rows [all obs | all actions] (its Q value)");
        hipLaunchKernelGGL(att_q_kernel, dim3((n_rows + e->h.rc - 1) / e->h.rc, e->h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
        HIP_TRY(hipGetLastError());
        return FRL_OK;
    }
    if (masac_actor && mode != FRL_ACT_RAW) {      // the stacked [mean | log_std] head (kernels_masac.hip); FRL_ACT_RAW and the critics: act_kernel below
        if ((mode != FRL_ACT_SAC_SAMPLE && mode != FRL_ACT_TANHHEAD) || ex) return fail(FRL_ERR_INVALID, "a MASAC actor acts through FRL_ACT_SAC_SAMPLE, FRL_ACT_TANHHEAD or FRL_ACT_RAW");
        if (mode == FRL_ACT_SAC_SAMPLE && !eps_dev) return fail(FRL_ERR_INVALID, "FRL_ACT_SAC_SAMPLE on a MASAC actor needs the N(0,1) draws in eps");
        hipLaunchKernelGGL(masac_act_kernel, dim3((n_rows + e->h.rc - 1) / e->h.rc, e->h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
        HIP_TRY(hipGetLastError());
        return FRL_OK;
    }
    if (e->h.algo == ALGO_CEM_GD3PG) {      // tanh actors and a LeakyReLU critic in one engine: kernels_cem_gd3pg.hip's forward
        const bool critic = net == 2;
        const bool ok = critic ? mode == FRL_ACT_RAW : (mode == FRL_ACT_TANHHEAD || mode == FRL_ACT_RAW);
        if (!ok || ex || (net == 3 && use_target))
            return fail(FRL_ERR_INVALID, "a CEM-GD3PG engine acts through FRL_ACT_TANHHEAD (nets 0, 1 and 3; use_target on 0 and 1) and FRL_ACT_RAW (net 2: Q of [obs | act])");
        hipLaunchKernelGGL(cem_act_kernel, dim3((n_rows + e->h.rc - 1) / e->h.rc, e->h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
        HIP_TRY(hipGetLastError());
        return FRL_OK;
    }
    if (gail_ppo) {      // LeakyReLU hidden layers and the engine's own log_std range: kernels_gail_ppo.hip's forward
        const bool disc = e->h.n_discrete > 0, actor = net == 0;
        const bool ok = mode == FRL_ACT_RAW || (actor && !disc && (mode == FRL_ACT_TANHHEAD || mode == FRL_ACT_PPO_SAMPLE)) ||
                        (actor && disc && (mode == FRL_ACT_CAT_SAMPLE || mode == FRL_ACT_ARGMAX));
        if (!ok || use_target || ex)
            return fail(FRL_ERR_INVALID, "a GAIL-PPO engine acts through FRL_ACT_RAW (either net, online), FRL_ACT_TANHHEAD / FRL_ACT_PPO_SAMPLE (continuous actor) or "
                                         "FRL_ACT_CAT_SAMPLE / FRL_ACT_ARGMAX (discrete actor)");
        if ((mode == FRL_ACT_PPO_SAMPLE || mode == FRL_ACT_CAT_SAMPLE) && !eps_dev) { a.device_eps = 1; a.rng_counter = e->rng_counter++; }      // Philox, as PPO's collectors draw
        hipLaunchKernelGGL(gail_ppo_act_kernel, dim3((n_rows + e->h.rc - 1) / e->h.rc, e->h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
        HIP_TRY(hipGetLastError());
        return FRL_OK;
    }
    if (e->h.algo == ALGO_GAIL) {      // LeakyReLU hidden layers: the discriminator's own forward kernel (kernels_gail.hip), logits of the online net
        if (mode != FRL_ACT_RAW || use_target || ex) return fail(FRL_ERR_INVALID, "a GAIL engine acts through FRL_ACT_RAW on its online net (the logits)");
        hipLaunchKernelGGL(gail_forward_kernel, dim3((n_rows + e->h.rc - 1) / e->h.rc, e->h.P), dim3(256), e->lds_bytes, e->stream, e->d, 0, n_rows, in_dev, out_dev);
        HIP_TRY(hipGetLastError());
        return FRL_OK;
    }
    if (N.frag && (e->h.wide || e->h.solow)) {
        // fragment-image parameters of a shape act_frag_kernel does not take: the net is re-laid out to Wk in a scratch copy (one
        // small launch: the actor of config 4 is 67 k floats per learner) and act_kernel reads that
        // (config 4 at 512 learners: 34 M floats per net — a collector that steps its envs many times between two learn() calls
        // pays the pass once per update, not once per vector step)
        const int slot = 2 * net + (use_target ? 1 : 0);
        float* wk = e->d_act_wk + (size_t)slot * e->act_wk_slot;
        if (!e->d_act_wk || slot >= (int)e->act_wk_version.size()) return fail(FRL_ERR_STATE, "wide engine without its act scratch");
        if (e->act_wk_version[slot] != e->param_version) {
            // (enough workgroups per learner for a few thousand elements each, the chip's CUs at most twice over)
            const int per = std::max(1, std::min((N.size + 2047) / 2048, 2 * e->n_cus / e->h.P));
            hipLaunchKernelGGL(frag_to_wk_kernel, dim3(e->h.P, per), dim3(256), 0, e->stream, e->d, net, use_target, wk);
            e->act_wk_version[slot] = e->param_version;
        }
        a.theta_alt = wk;
        dim3 grid((n_rows + e->h.rc - 1) / e->h.rc, e->h.P);
        hipLaunchKernelGGL(act_kernel, grid, dim3(256), e->lds_bytes, e->stream, e->d, a);
    } else if (N.frag) {       // parameters in fragment-image order: the register-chained forward (kernels_act.hip)
        hipLaunchKernelGGL(act_frag_kernel, dim3((n_rows + 63) / 64, e->h.P), dim3(256), (size_t)critic2_lds_floats() * sizeof(float),
                           e->stream, e->d, a);
    } else {
        dim3 grid((n_rows + e->h.rc - 1) / e->h.rc, e->h.P);
        hipLaunchKernelGGL(act_kernel, grid, dim3(256), e->lds_bytes, e->stream, e->d, a);
    }
    HIP_TRY(hipGetLastError());
    return FRL_OK;
}

extern "C" int frl_act_device(frl_engine* e, int net, int mode, int head, int use_target, int n_rows, int in_dim,
                              const float* in_dev, const float* eps_dev, float* out_dev, float* logp_dev) {
    ENG(e);
    if (!in_dev || !out_dev) return fail(FRL_ERR_INVALID, "NULL device buffer");
    return launch_act(e, net, mode, head, use_target, n_rows, in_dim, in_dev, eps_dev, out_dev, logp_dev);
}

// The host-facing act entry points' device scratch (frl_act, frl_act_explore, frl_gail_reward): the input rows, and eps / out / logp
// of out_n floats each.  Buffers only grow; one that could not holds nothing, and the next call allocates it again
static int act_scratch(frl_engine* e, size_t in_n, size_t out_n) {
    HIP_TRY(e->mem.grow(&e->d_act_in, e->act_in_cap, in_n, MEM_DEVICE));
    HIP_TRY(e->mem.grow(&e->d_act_eps, e->act_eps_cap, out_n, MEM_DEVICE));
    HIP_TRY(e->mem.grow(&e->d_act_out, e->act_out_cap, out_n, MEM_DEVICE));
    HIP_TRY(e->mem.grow(&e->d_act_logp, e->act_logp_cap, out_n, MEM_DEVICE));
    return FRL_OK;
}

extern "C" int frl_act(frl_engine* e, int net, int mode, int head, int use_target, int n_rows, int in_dim,
                       const float* in_host, const float* eps_host, float* out_host, float* logp_host) {
    ENG(e);
    if (!e->has_nets) return fail(FRL_ERR_STATE, "replay-only engine has no networks");
    if (net < 0 || net >= e->h.n_nets) return fail(FRL_ERR_INVALID, "net %d out of range", net);
    if (!in_host || !out_host || n_rows < 1) return fail(FRL_ERR_INVALID, "bad argument");
    const NetDesc& N = e->h.net[net];
    const int nl = N.n_layers / N.heads;
    if (head < 0 || head >= N.heads) return fail(FRL_ERR_INVALID, "head out of range");
    int nout = N.L[head * nl + nl - 1].n;
    if (e->h.algo == ALGO_MASAC && !(net & 1) && (mode & ~FRL_ACT_NO_OBSNORM) != FRL_ACT_RAW) nout /= 2;      // an action, not the [mean | log_std] head row
    const size_t rows = (size_t)e->h.P * n_rows;
    const size_t in_n = rows * in_dim, out_n = rows * nout;
    int rc = act_scratch(e, in_n, out_n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_act_in, in_host, in_n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (eps_host) HIP_TRY(hipMemcpyAsync(e->d_act_eps, eps_host, out_n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    rc = launch_act(e, net, mode, head, use_target, n_rows, in_dim, e->d_act_in, eps_host ? e->d_act_eps : nullptr,
                        e->d_act_out, logp_host ? e->d_act_logp : nullptr);
    if (rc) return rc;
    const int base_mode = mode & ~FRL_ACT_NO_OBSNORM;
    const bool one_per_row = (base_mode == FRL_ACT_ARGMAX || base_mode == FRL_ACT_CAT_SAMPLE);
    const size_t got = one_per_row ? rows : out_n;
    HIP_TRY(hipMemcpyAsync(out_host, e->d_act_out, got * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (logp_host) HIP_TRY(hipMemcpyAsync(logp_host, e->d_act_logp, got * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return FRL_OK;
}

// select_action + the reference loop's exploration rule in ONE launch, host in / host out (tests, single-env callers): the
// rollout collectors use the same launch with device-resident buffers.  mode: FRL_ACT_ARGMAX (+ epsilon-greedy),
// FRL_ACT_TANHHEAD / FRL_ACT_SAC_SAMPLE (+ Gaussian or OU action noise, or none).  Sampling modes draw their own eps.
extern "C" int frl_act_explore(frl_engine* e, int mode, int n_rows, const float* obs_host, const frl_explore_args* x,
                               const uint8_t* ended_host, float* store_act_out, float* env_act_out) {
    ENG(e);
    if (!e->has_nets) return fail(FRL_ERR_STATE, "replay-only engine has no networks");
    if (!obs_host || !x || !store_act_out || !env_act_out || n_rows < 1) return fail(FRL_ERR_INVALID, "bad argument");
    const EngineDesc& h = e->h;
    if (is_mappo_family(h.algo)) return wrong_engine(h, "frl_act_explore");
    if (h.algo == ALGO_MASAC) return fail(FRL_ERR_STATE, "frl_act_explore does not serve a MASAC engine: %s", algo_traits(h.algo).act_hint);
    if (h.n_agents != 1) return fail(FRL_ERR_STATE, "frl_act_explore: single-agent engines");
    if (*algo_traits(h.algo).act_hint) return wrong_engine(h, "frl_act_explore");
    const int O = h.rec.obs_dim[0], nout = h.net[0].L[h.net[0].n_layers / h.net[0].heads - 1].n;
    const bool disc = (mode == FRL_ACT_ARGMAX);
    const size_t rows = (size_t)h.P * n_rows, in_n = rows * O, out_n = rows * nout;
    int rc = act_scratch(e, in_n, out_n);
    if (rc) return rc;
    if (out_n != e->ou_n) {                 // OU state of the host-facing entry point: one process per (learner, row, dimension)
        e->ou_n = 0;
        HIP_TRY(e->mem.alloc_zero(&e->d_ou, out_n, e->stream));
        HIP_TRY(e->mem.alloc(&e->d_ou_flags, rows, MEM_DEVICE));
        e->ou_n = out_n;
    }
    HIP_TRY(hipMemcpyAsync(e->d_act_in, obs_host, in_n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (ended_host) {
        std::vector<unsigned char> fl(rows);
        for (size_t i = 0; i < rows; ++i) fl[i] = ended_host[i] ? 2 : 0;
        HIP_TRY(hipMemcpy(e->d_ou_flags, fl.data(), rows, hipMemcpyHostToDevice));
    }
    ActExplore ex;
    ex.x = *x; ex.ou_state_dev = e->d_ou; ex.flags_dev = ended_host ? e->d_ou_flags : nullptr;
    ex.env_out_dev = e->d_act_eps;           // scratch of the same size, unused by a device_eps launch
    ex.device_eps = true;
    rc = launch_act(e, 0, mode, 0, 0, n_rows, O, e->d_act_in, nullptr, e->d_act_out, nullptr, &ex);
    if (rc) return rc;
    const size_t got = disc ? rows : out_n;
    HIP_TRY(hipMemcpyAsync(store_act_out, e->d_act_out, got * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(env_act_out, e->d_act_eps, got * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return FRL_OK;
}

// ------------------------------------------------------------------------------------ learn
static int upload_idx_noise(frl_engine* e, const int64_t* idx, const float* noise, int batch, int n_sets_per_learner) {
    const EngineDesc& h = e->h;
    if (idx || noise) HIP_TRY(hipStreamSynchronize(e->stream));    // pinned scratch reuse
    if (idx) {
        for (int p = 0; p < h.P; ++p)
            for (int a = 0; a < n_sets_per_learner; ++a) {
                const int64_t* src = idx + ((size_t)p * n_sets_per_learner + a) * batch;
                int* dst = e->h_idx + ((size_t)p * h.n_agents + a) * h.batch_max;
                const int sz = e->size[p];
                for (int i = 0; i < batch; ++i) {
                    int64_t v = src[i];
                    if (v < 0) v += h.capacity;
                    if (v < 0 || v >= h.capacity) return fail(FRL_ERR_INVALID, "sample index %lld out of range", (long long)src[i]);
                    (void)sz;
                    dst[i] = (int)v;
                }
            }
        HIP_TRY(hipMemcpyAsync(h.idx, e->h_idx, e->idx_count * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    if (noise) {
        // host [P][n_agents][noise_sets][batch][act_max] -> device [P][n_agents][noise_sets][batch_max][act_max]
        const int am = h.act_max;
        for (size_t s = 0; s < (size_t)h.P * h.n_agents * h.noise_sets; ++s)
            memcpy(e->h_noise + s * h.batch_max * am, noise + s * batch * am, (size_t)batch * am * sizeof(float));
        HIP_TRY(hipMemcpyAsync(h.noise, e->h_noise, e->noise_count * sizeof(float), hipMemcpyHostToDevice, e->stream));
    }
    return FRL_OK;
}

extern "C" int frl_stats_get(frl_engine* e, float* out_host) {
    ENG(e);
    if (!e->has_nets || !out_host) return fail(FRL_ERR_INVALID, "bad argument");
    HIP_TRY(hipMemcpyAsync(out_host, e->h.stats, (size_t)e->h.P * e->h.n_agents * ST_COUNT * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return solo_err_check(e);
}

// What a learn entry point of its own hands back once its launches are enqueued: [the preference vectors used, weight_num per learner,]
// and up to two statistics per learner out of one copy of h.stats, after one synchronise (which also lands what the caller enqueued).
// written: per learner, > 0 = write its statistics (nullptr: everybody's)
struct StatOut { int slot; float* out; };
static int read_back(frl_engine* e, float* weights_out, int weight_num, StatOut s0, StatOut s1 = {0, nullptr}, const int* written = nullptr) {
    const EngineDesc& h = e->h;
    const size_t wpitch = (size_t)h.batch_max * h.reward_dim, wn = (size_t)weight_num * h.reward_dim;
    for (int p = 0; weights_out && p < h.P; ++p)
        HIP_TRY(hipMemcpyAsync(weights_out + p * wn, h.env_w + p * wpitch, wn * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    std::vector<float> st;
    if (s0.out || s1.out) {
        st.resize((size_t)h.P * ST_COUNT);
        HIP_TRY(hipMemcpyAsync(st.data(), h.stats, st.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (const StatOut& s : {s0, s1})
        for (int p = 0; s.out && p < h.P; ++p)
            if (!written || written[p] > 0) s.out[p] = st[(size_t)p * ST_COUNT + s.slot];
    return FRL_OK;
}

extern "C" int frl_last_indices(frl_engine* e, int batch, int64_t* out_host) {
    ENG(e);
    if (!e->has_nets || !out_host || batch < 1 || batch > e->h.batch_max) return fail(FRL_ERR_INVALID, "bad argument");
    const size_t units = (size_t)e->h.P * e->h.n_agents;
    std::vector<int> tmp(units * e->h.batch_max);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(tmp.data(), e->h.idx, tmp.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t u = 0; u < units; ++u)
        for (int i = 0; i < batch; ++i) out_host[u * batch + i] = tmp[u * e->h.batch_max + i];
    return FRL_OK;
}

// Host noise of `n_sets` forwards -> the device layout of kernels_noisy.hip.  Host order per forward (frl_noisy_eps_size
// floats): per NoisyLinear eps_in[hidden] then eps_out[rows], V before A for a Dueling head.
static int noisy_upload(frl_engine* e, const float* eps_host, int set0, int n_sets) {
    const EngineDesc& h = e->h;
    const LayerDesc& H = h.net[0].L[h.net[0].n_layers - 1];
    const int per = e->noisy_per_set, K = H.k, kp = H.k_pad, np_ = H.n_pad;
    const int rows0 = h.dueling ? h.noisy_split : H.n, rows1 = h.dueling ? H.n - h.noisy_split : 0;
    const int host_per = K + rows0 + (rows1 ? K + rows1 : 0);
    HIP_TRY(hipStreamSynchronize(e->stream));                       // pinned staging reuse
    for (int p = 0; p < h.P; ++p)
        for (int s = 0; s < n_sets; ++s) {
            const float* src = eps_host + ((size_t)p * n_sets + s) * host_per;
            float* dst = e->h_noisy + ((size_t)p * 3 + set0 + s) * per;
            memset(dst, 0, (size_t)per * sizeof(float));
            memcpy(dst, src, (size_t)K * sizeof(float));                                   // eps_in of sub-layer 0
            memcpy(dst + kp, src + K, (size_t)rows0 * sizeof(float));                      // eps_out of sub-layer 0: rows [0, rows0)
            if (rows1) {
                memcpy(dst + kp + np_, src + K + rows0, (size_t)K * sizeof(float));        // eps_in of sub-layer 1
                memcpy(dst + kp + np_ + kp + rows0, src + K + rows0 + K, (size_t)rows1 * sizeof(float));   // rows [rows0, n)
            }
        }
    for (int p = 0; p < h.P; ++p)
        HIP_TRY(hipMemcpyAsync(h.noisy_eps + ((size_t)p * 3 + set0) * per, e->h_noisy + ((size_t)p * 3 + set0) * per,
                               (size_t)n_sets * per * sizeof(float), hipMemcpyHostToDevice, e->stream));
    return FRL_OK;
}

extern "C" int frl_noisy_eps_size(const frl_engine* e, int* n_out) {
    if (!e || !n_out) return fail(FRL_ERR_INVALID, "NULL argument");
    *n_out = 0;
    if (!e->h.noisy) return FRL_OK;
    const EngineDesc& h = e->h;
    const LayerDesc& H = h.net[0].L[h.net[0].n_layers - 1];
    const int rows0 = h.dueling ? h.noisy_split : H.n, rows1 = h.dueling ? H.n - h.noisy_split : 0;
    *n_out = H.k + rows0 + (rows1 ? H.k + rows1 : 0);
    return FRL_OK;
}

// A forward of the online net with fresh noise (select_action on a noisy net, DQN_with_tricks.py:213-216 with
// Noisy_net.py:41-44): materialises effective set 0; frl_act(..., use_target = 2, ...) then reads it.
extern "C" int frl_noisy_resample(frl_engine* e, const float* eps_host) {
    ENG(e);
    if (!e->h.noisy) return fail(FRL_ERR_STATE, "engine has no NoisyLinear head");
    if (eps_host) { int rc = noisy_upload(e, eps_host, 0, 1); if (rc) return rc; }
    else hipLaunchKernelGGL(noisy_draw_kernel, dim3(e->h.P, 1), dim3(256), 0, e->stream, e->d, 0, 1, e->rng_counter++);
    hipLaunchKernelGGL(noisy_materialise_kernel, dim3(e->h.P), dim3(256), 0, e->stream, e->d, 0, 1, 0);
    HIP_TRY(hipGetLastError());
    return FRL_OK;
}

#include "frl_api_learn.inc"

// developer read-back (tools/solo_timing.py): the single-learner kernels' per-workgroup partial sums and, in a -DFRL_SOLO_TIMING build of
// kernels_solo.hip, their section stamps — [kSoloWG][32] floats of learner 0
extern "C" int frl_solo_debug_read(frl_engine* e, float* out_host, int n_floats) {
    ENG(e);
    if (!(e->h.solo || e->h.solow) || !e->d_solo_part || !out_host || n_floats < 0 || n_floats > kSoloWG * kSoloPartHost) return fail(FRL_ERR_STATE, "not a solo engine / bad size");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out_host, e->d_solo_part, (size_t)n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return FRL_OK;
}

// ----------------------------------------------------------------------------------- timing
extern "C" int frl_timer_start(frl_engine* e) {
    ENG(e);
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    return FRL_OK;
}
extern "C" int frl_timer_stop(frl_engine* e, float* ms_out) {
    ENG(e);
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    HIP_TRY(hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    if (ms_out) *ms_out = ms;
    return FRL_OK;
}

// Batch_ObsNorm (Normalization_batch_size): switch + statistics {n, mean[O], S[O], std[O]} per learner
extern "C" int frl_obsnorm_enable(frl_engine* e, int on) {
    ENG(e);
    if (!e->has_nets) return fail(FRL_ERR_STATE, "replay-only engine has no networks");
    if (e->h.algo == ALGO_MASAC) return fail(FRL_ERR_STATE, "frl_obsnorm_enable: MASAC.py has no Batch_ObsNorm and kernels_masac.hip does not normalise");
    if (e->h.algo == ALGO_CEM_GD3PG) return fail(FRL_ERR_STATE, "frl_obsnorm_enable: CEM_GD3PG.py has no Batch_ObsNorm and kernels_cem_gd3pg.hip does not normalise");
    if (e->h.algo == ALGO_GAIL_PPO) return fail(FRL_ERR_STATE, "frl_obsnorm_enable: PPO2.py has no Batch_ObsNorm (its env wrapper scales observations) and kernels_gail_ppo.hip does not normalise");
    if (e->h.algo == ALGO_MADDPG_ATT) return fail(FRL_ERR_STATE, "frl_obsnorm_enable: MADDPG_simple_with_tricks.py has no Batch_ObsNorm and the attention critic's kernels do not normalise");
    if (is_mappo_family(e->h.algo)) return wrong_engine(e->h, "frl_obsnorm_enable");      // (ObsNorm belongs to these algorithms' loop: freerl_amd/normalization.py)
    if (on && e->h.net[0].frag) {
        // Batch_ObsNorm belongs to the row-chunk family: an engine created for the register-chained kernels (parameters in
        // fragment-image order) moves over for good — every parameter array back to Wk, through a scratch copy
        float* scratch = nullptr;
        HIP_TRY(hipMalloc((void**)&scratch, (size_t)4 * e->h.P * e->h.learner_stride * sizeof(float)));
        hipLaunchKernelGGL(relayout_to_wk_kernel, dim3(e->h.P, 4), dim3(256), 0, e->stream, e->d, scratch);
        hipError_t he = hipStreamSynchronize(e->stream);
        hipFree(scratch);
        if (he != hipSuccess) return fail(FRL_ERR_HIP, "relayout: %s", hipGetErrorString(he));
        for (int i = 0; i < e->h.n_nets; ++i) e->h.net[i].frag = 0;
        ++e->param_version;
        e->family = FAM_ROWCHUNK;
        e->h.wide = 0;
        e->h.solo = 0;
        e->h.solow = 0;
    }
    e->h.obs_norm_on = on ? 1 : 0;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->d, &e->h, sizeof e->h, hipMemcpyHostToDevice));
    return FRL_OK;
}
// stats of one learner: n_agents blocks of (1 + 3*max obs_dim) floats, block j = {n, mean[O_j], S[O_j], std[O_j]} of agent j
// (the version the next select_action / learn starts from); single agent: one block of 1 + 3*O floats
static float* obsnorm_final(frl_engine* e, int learner) {
    const size_t n = e->h.n_agents, w = e->h.obsnorm_w;
    return e->h.obsnorm + (((size_t)learner * n + (n - 1)) * n) * w;
}
extern "C" int frl_obsnorm_get(frl_engine* e, int learner, float* stats_out) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || !stats_out) return fail(FRL_ERR_INVALID, "bad argument");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(stats_out, obsnorm_final(e, learner), (size_t)e->h.n_agents * e->h.obsnorm_w * sizeof(float), hipMemcpyDeviceToHost));
    return FRL_OK;
}
extern "C" int frl_obsnorm_set(frl_engine* e, int learner, const float* stats) {
    ENG(e);
    if (!e->has_nets || learner < 0 || learner >= e->h.P || !stats) return fail(FRL_ERR_INVALID, "bad argument");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(obsnorm_final(e, learner), stats, (size_t)e->h.n_agents * e->h.obsnorm_w * sizeof(float), hipMemcpyHostToDevice));
    return FRL_OK;
}

extern "C" int frl_profile_enable(frl_engine* e, int on) {
    ENG(e);
    prof_collect(e);
    e->profile = on != 0;
    if (on) { for (int k = 0; k < 8; ++k) { e->prof_ms[k] = 0; e->prof_n[k] = 0; } }
    return FRL_OK;
}
extern "C" int frl_profile_read(frl_engine* e, double* ms_sum8, long long* count8) {
    ENG(e);
    prof_collect(e);
    for (int k = 0; k < 8; ++k) { if (ms_sum8) ms_sum8[k] = e->prof_ms[k]; if (count8) count8[k] = e->prof_n[k]; }
    return FRL_OK;
}

// ------------------------------------------------------------------------- prioritised replay
extern "C" int frl_per_enable(frl_engine* e, double alpha, double beta, double beta_increment, double epsilon) {
    ENG(e);
    if (e->h.n_agents != 1) return fail(FRL_ERR_INVALID, "PER is a single-agent buffer (DQN_file/Buffer.py:66)");
    if (e->per_on) return fail(FRL_ERR_STATE, "PER already enabled");
    if (e->n_rings != 1) return fail(FRL_ERR_STATE, "frl_per_enable: a %s engine samples its two rings uniformly (CEM_GD3PG.py:160-176)", algo_traits(e->h.algo).name);
    int rc = flush_stage(e);
    if (rc) return rc;
    for (int p = 0; p < e->h.P; ++p)
        if (e->size[p] != 0) return fail(FRL_ERR_STATE, "enable PER on an empty buffer (priorities are assigned by add)");
    const size_t nn = 2 * (size_t)e->h.capacity - 1, P = e->h.P;
    const size_t bm = (size_t)std::max(e->h.batch_max, 1), bucket_n = 2 * P + 1 + (size_t)e->stage_cap;
    const bool replay_only = !e->h.isw;       // Buffer.py's PER_Buffer on its own: sample rows, weights and TD errors still need a home
    const size_t mark = e->mem.live();
    auto allocate = [&]() -> int {
        HIP_TRY(e->mem.alloc_zero(&e->d_per_sum, P * nn, e->stream));
        HIP_TRY(e->mem.alloc_zero(&e->d_per_max, P * nn, e->stream));
        HIP_TRY(e->mem.alloc(&e->d_size, 2 * P, MEM_DEVICE));
        HIP_TRY(e->mem.alloc(&e->d_stage_bucket, bucket_n, MEM_DEVICE));
        HIP_TRY(e->mem.alloc(&e->stage_bucket, bucket_n, MEM_PINNED));
        HIP_TRY(e->mem.alloc(&e->d_per_prio, P * bm, MEM_DEVICE));
        HIP_TRY(e->mem.alloc(&e->d_uniforms, P * bm, MEM_DEVICE));
        if (replay_only) {
            HIP_TRY(e->mem.alloc(&e->h.isw, P * bm, MEM_DEVICE));
            HIP_TRY(e->mem.alloc(&e->h.td_err, P * bm, MEM_DEVICE));
            e->idx_count = P * e->h.n_agents * bm;
            HIP_TRY(e->mem.alloc(&e->h.idx, e->idx_count, MEM_DEVICE));
            HIP_TRY(e->mem.alloc(&e->h_idx, e->idx_count, MEM_PINNED));
            HIP_TRY(hipMemcpy(e->d, &e->h, sizeof(EngineDesc), hipMemcpyHostToDevice));
        }
        return FRL_OK;
    };
    rc = allocate();
    if (rc) {                 // nothing of a failed call stays: a retry starts from empty slots
        e->mem.release_to(mark);
        return rc;
    }
    e->per_alpha = (float)alpha; e->per_beta = beta; e->per_beta_inc = beta_increment; e->per_eps = (float)epsilon;
    e->size_flushed.assign(P, 0);
    e->per_on = true;
    return FRL_OK;
}

extern "C" int frl_per_sample(frl_engine* e, int batch, const double* uniforms, int64_t* idx_out, float* is_weight_out) {
    ENG(e);
    if (!e->per_on) return fail(FRL_ERR_STATE, "frl_per_enable first");
    if (batch < 1 || batch > e->h.batch_max) return fail(FRL_ERR_INVALID, "batch %d outside [1,%d]", batch, e->h.batch_max);
    int rc = flush_stage(e);
    if (rc) return rc;
    const size_t P = e->h.P;
    for (size_t p = 0; p < P; ++p)
        if (e->size[p] < 1) return fail(FRL_ERR_STATE, "learner %zu's buffer is empty", p);
    e->per_beta = std::min(1.0, e->per_beta + e->per_beta_inc);             // Buffer.py:105 (before the weights are computed)
    HIP_TRY(hipMemcpyAsync(e->d_size + P, e->size.data(), P * sizeof(int), hipMemcpyHostToDevice, e->stream));
    if (uniforms) HIP_TRY(hipMemcpyAsync(e->d_uniforms, uniforms, P * batch * sizeof(double), hipMemcpyHostToDevice, e->stream));
    PerArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.sum_tree = e->d_per_sum; pa.max_tree = e->d_per_max; pa.cap = e->h.capacity; pa.n = batch;
    pa.size = e->d_size + P; pa.uniforms = uniforms ? e->d_uniforms : nullptr; pa.isw = e->h.isw; pa.prio_out = e->d_per_prio;
    pa.beta = e->per_beta; pa.rng_counter = e->rng_counter++;
    hipLaunchKernelGGL(per_sample_kernel, dim3((unsigned)P), dim3(256), 0, e->stream, e->d, pa);
    HIP_TRY(hipGetLastError());
    if (!idx_out && !is_weight_out) return FRL_OK;            // device-resident use (frl_learn with per = 1): asynchronous
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t bm = e->h.batch_max;
    if (idx_out) {
        std::vector<int> tmp(bm * P);
        HIP_TRY(hipMemcpy(tmp.data(), e->h.idx, tmp.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < P; ++p)
            for (int i = 0; i < batch; ++i) idx_out[p * batch + i] = tmp[p * bm + i];
    }
    if (is_weight_out) {
        std::vector<float> tmp(bm * P);
        HIP_TRY(hipMemcpy(tmp.data(), e->h.isw, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < P; ++p) memcpy(is_weight_out + p * batch, tmp.data() + p * bm, (size_t)batch * sizeof(float));
    }
    return FRL_OK;
}

extern "C" int frl_per_update(frl_engine* e, int batch, const int64_t* idx, const float* td_error) {
    ENG(e);
    if (!e->per_on) return fail(FRL_ERR_STATE, "frl_per_enable first");
    if (batch < 1 || batch > e->h.batch_max) return fail(FRL_ERR_INVALID, "batch %d outside [1,%d]", batch, e->h.batch_max);
    if (batch > kPerSetMax) return fail(FRL_ERR_INVALID, "priority update of %d rows: at most %d per call (split the batch)", batch, kPerSetMax);
    int rc = flush_stage(e);
    if (rc) return rc;
    const size_t P = e->h.P, bm = e->h.batch_max;
    if (idx) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (size_t p = 0; p < P; ++p)
            for (int i = 0; i < batch; ++i) {
                const int64_t v = idx[p * batch + i];
                if (v < 0 || v >= e->h.capacity) return fail(FRL_ERR_INVALID, "priority index %lld out of range", (long long)v);
                e->h_idx[p * bm + i] = (int)v;
            }
        HIP_TRY(hipMemcpyAsync(e->h.idx, e->h_idx, P * bm * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    if (td_error)
        for (size_t p = 0; p < P; ++p)
            HIP_TRY(hipMemcpyAsync(e->h.td_err + p * bm, td_error + p * batch, (size_t)batch * sizeof(float), hipMemcpyHostToDevice, e->stream));
    PerArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.sum_tree = e->d_per_sum; pa.max_tree = e->d_per_max; pa.cap = e->h.capacity; pa.n = batch;
    pa.leaf = e->h.idx; pa.n_pitch = (int)bm; pa.td = e->h.td_err; pa.alpha = e->per_alpha; pa.eps = e->per_eps;
    hipLaunchKernelGGL(per_set_kernel, dim3((unsigned)P), dim3(256), 0, e->stream, e->d, pa);
    HIP_TRY(hipGetLastError());
    return FRL_OK;
}

extern "C" int frl_per_state(frl_engine* e, int learner, double* sum_out, double* max_out, double* beta_out) {
    ENG(e);
    if (!e->per_on) return fail(FRL_ERR_STATE, "frl_per_enable first");
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner out of range");
    int rc = flush_stage(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t nn = 2 * (size_t)e->h.capacity - 1;
    if (sum_out) HIP_TRY(hipMemcpy(sum_out, e->d_per_sum + learner * nn, sizeof(double), hipMemcpyDeviceToHost));
    if (max_out) HIP_TRY(hipMemcpy(max_out, e->d_per_max + learner * nn, sizeof(double), hipMemcpyDeviceToHost));
    if (beta_out) *beta_out = e->per_beta;
    return FRL_OK;
}

#ifdef FRL_PHASE_TIMING
// developer build only (tools/phase_timing.py): not part of include/freerl_hip.h
extern "C" int frl_debug_phase_clocks(int* out, int stride) {
    if (stride < 0) { const int k = -stride - 1; return (int)hipMemcpyToSymbol(HIP_SYMBOL(frl::g_phase_kernel), &k, sizeof(int), 0, hipMemcpyHostToDevice); }
    if (stride > 0) return (int)hipMemcpyToSymbol(HIP_SYMBOL(frl::g_phase_stride), &stride, sizeof(int), 0, hipMemcpyHostToDevice);
    hipDeviceSynchronize();
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(frl::g_phase_clock), sizeof(int) * frl::kPhaseBlocks * frl::kPhaseWords, 0,
                                    hipMemcpyDeviceToHost);
}
#endif
#include "frl_api_ppo.inc"
#include "frl_api_reinforce.inc"
#include "frl_api_envelope.inc"
#include "frl_api_envelope_ddpg.inc"
#include "frl_api_gail.inc"
#include "frl_api_gail_ppo.inc"
#include "frl_api_mappo.inc"
#include "frl_api_happo.inc"
#include "frl_api_rollout.inc"
#include "frl_api_her.inc"
#include "frl_api_comm.inc"
#include "frl_api_cem_gd3pg.inc"
