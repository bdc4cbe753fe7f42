// What a frl_rollout call decides before it touches the device: which calls are refused, the exploration rule, and how the vector
// step reaches the device — folded into the learn launch or not, the block read in place, the flagged hand-over, pre-armed launches.
// Arithmetic on the engine's and the pool's facts, the call's arguments and the per-call knobs — plain C++17, no HIP, no getenv — so
// tests/rollout_plan_probe.cpp states every rule on the CPU (tests/test_rollout_plan.py).  frl_api_rollout.inc gathers the facts, reads
// the knobs (rollout_knobs), calls plan_rollout and runs the loop the plan says.
#pragma once
#include "engine_plan.hpp"

namespace frl {

// The per-call developer / test knobs (read at EVERY call: the tests flip them between calls of one process).  A tri-state is -1 unset,
// 0 or 1; knob_flag() applies its default.
struct RolloutKnobs {
    bool timing = false;            // FRL_ROLLOUT_TIMING (set at all): host wall time of the loop's sections on stderr
    bool dqn_step_fuse = true;      // FRL_DQN_STEP_FUSE=0: the separate commit / learn / act launches, same draws
    bool solo_step_fuse = true;     // FRL_SOLO_STEP_FUSE=0: the same for the single-learner kernels
    int zero_copy = -1;             // FRL_ROLLOUT_ZEROCOPY (tri-state; unset: blocks of up to 64 KiB)
    bool poll = true;               // FRL_ROLLOUT_POLL=0: stream synchronisation instead of the flagged hand-over
    int prearm = -1;                // FRL_ROLLOUT_PREARM (tri-state; unset: the population bounds below, 1: past them, 0: never)
    double arm_patience_ms = 1000.0;   // FRL_ROLLOUT_ARM_PATIENCE_MS (tests: 0 = every armed launch is cancelled and replayed)
};

// What the decisions need from the engine — family: learn_family(e, args.learn.batch), what this call's frl_learn would run on; solo:
// EngineDesc::solo, workgroups per learner of kernels_solo.hip — and from the pool (blk_bytes: BlkLayout::bytes)
struct RolloutFacts {
    int algo = ALGO_DQN, P = 1, capacity = 0, n_discrete = 0, rec_obs_dim = 0, rec_act_dim = 0, n_cus = 256, solo = 0;
    bool per_on = false, profile = false;
    LearnFamily family = FAM_ROWCHUNK;
    int n = 0, obs_dim = 0, act_dim = 0, n_actions = 0;
    bool discrete = false;
    float max_action = 1.f;
    size_t blk_bytes = 0;
};

// kind: the resolved exploration rule; mode: of the act launch; aout: columns of the action add() stores; dev: exploration inside the act
// launch, records assembled on the device; host_commit: the records go through the staged add path; fold: add(), learn() and the next
// select_action in the learn launches; arm_patience: seconds
enum RolloutFold { FOLD_NONE, FOLD_DQN, FOLD_SOLO };
struct RolloutPlan {
    int kind = FRL_EXPLORE_NONE, mode = FRL_ACT_ARGMAX, aout = 1;
    float ma = 1.f;
    bool dev = true, host_commit = false, zero_copy = false, poll = false, prearm = false, timing = false;
    RolloutFold fold = FOLD_NONE;
    double arm_patience = 1.0;
};

// FRL_OK and *out, or the refusal's code and *message.  (That the engine is one frl_rollout collects for at all is said in front of this,
// by frl_rollout itself: wrong_engine.)
inline int plan_rollout(const RolloutFacts& f, const RolloutKnobs& k, const frl_rollout_args& ra, RolloutPlan* out, std::string* message) {
    const int E = ra.envs_per_learner;
    if (E < 1 || f.n != f.P * E) return plan_refuse(message, "pool has %d envs, engine needs P*E = %d*%d", f.n, f.P, E);
    if (E > f.capacity) return plan_refuse(message, "a vector step adds E = %d rows to a ring of %d", E, f.capacity);
    if (f.obs_dim != f.rec_obs_dim) return plan_refuse(message, "obs_dim mismatch (%d vs %d)", f.obs_dim, f.rec_obs_dim);
    const bool dqn = f.algo == ALGO_DQN, sac = f.algo == ALGO_SAC;
    if (dqn != f.discrete) return plan_refuse(message, "DQN needs a discrete env and the others a continuous one");
    if (!dqn && f.act_dim != f.rec_act_dim) return plan_refuse(message, "act_dim mismatch");
    if (dqn && f.n_actions != f.n_discrete) return plan_refuse(message, "n_actions mismatch");
    if (ra.learn.idx || ra.learn.noise) return plan_refuse(message, "rollout draws on the device: learn.idx/noise must be NULL");
    // a PER engine's priorities move with every sample: the loop of DQN_with_tricks.py (sample -> learn -> update_priorities)
    if (f.per_on && ra.learn_every > 0 && !ra.learn.per)
        return plan_refuse(message, "PER engine: set learn.per (1 reference weighting, 2 per-sample) so the rollout samples and updates priorities"), FRL_ERR_STATE;
    if (!f.per_on && ra.learn.per) return plan_refuse(message, "learn.per needs frl_per_enable"), FRL_ERR_STATE;
    RolloutPlan pl;
    pl.kind = ra.explore_kind;
    // 0 = what a memset-zero caller passes: the reference loop's own rule, never a silent "no exploration"
    if (pl.kind <= 0) pl.kind = dqn ? FRL_EXPLORE_EPS_GREEDY : (sac ? FRL_EXPLORE_NONE : FRL_EXPLORE_GAUSS);
    else if (pl.kind == FRL_EXPLORE_OFF) pl.kind = FRL_EXPLORE_NONE;
    else if (pl.kind > FRL_EXPLORE_OU) return plan_refuse(message, "unknown exploration kind %d", pl.kind);
    if (dqn != (pl.kind == FRL_EXPLORE_EPS_GREEDY))
        return plan_refuse(message, "epsilon-greedy is the discrete rule, Gaussian / OU / none the continuous ones");
    if (ra.host_explore && pl.kind == FRL_EXPLORE_OU) return plan_refuse(message, "OU exploration runs on the device path only");
    pl.mode = dqn ? FRL_ACT_ARGMAX : (sac ? FRL_ACT_SAC_SAMPLE : FRL_ACT_TANHHEAD);
    pl.aout = dqn ? 1 : f.act_dim;
    pl.ma = dqn ? 1.f : f.max_action;
    pl.dev = !ra.host_explore;
    pl.host_commit = !pl.dev || f.per_on;     // PER: priorities enter through the staged add path
    const bool on_device = pl.dev && !pl.host_commit;
    // DQN on the one-launch update (kernels_dqn2.hip): add(), learn() and the next step's select_action + epsilon-greedy are
    // ONE launch per vector step (FRL_DQN_STEP_FUSE=0: the separate commit / learn / act launches, same draws)
    if (k.dqn_step_fuse && on_device && dqn && f.family == FAM_DQN_FUSED) pl.fold = FOLD_DQN;
    // DDPG / TD3 / SAC on the single-learner kernels (kernels_solo.hip): the same fold — add() at the head of the critic launch, the
    // next select_action + exploration at the tail of the step's last launch (FRL_SOLO_STEP_FUSE=0: the separate launches, same draws)
    if (k.solo_step_fuse && on_device && !dqn && f.family == FAM_SOLO && E <= 1024) pl.fold = FOLD_SOLO;
    // small vector steps: the launch reads the pinned block and writes the env actions in host memory directly (hipHostMalloc
    // memory is device-visible and coherent at kernel boundaries) — a hipMemcpyAsync each way costs more than the launch itself
    // (measured at one env: 58 us from enqueue to the actions on the host for a 28 us launch).  FRL_ROLLOUT_ZEROCOPY=0/1 overrides.
    pl.zero_copy = on_device && knob_flag(k.zero_copy, f.blk_bytes <= 64 * 1024);
    // ... and the host picks the actions up as soon as the launch has flagged them (a release store to a pinned word after
    // the action stores) instead of waiting for the launch to retire and the runtime to notice.  FRL_ROLLOUT_POLL=0: stream sync.
    pl.poll = pl.zero_copy && pl.fold != FOLD_NONE && k.poll;
    // PRE-ARMED launches (small populations on the folded step with the flagged hand-over): the launch of step t + 1 is enqueued as
    // soon as step t's doorbell is rung, on the OTHER of two streams — its arguments are all predictable (ring sizes grow by E per
    // step, Philox counters by two).  It starts while step t's launch runs, draws its rows, waits on a device word for step t's
    // launches to have left, stages its nets and spins on a doorbell word; the host, back from env.step with the block filled, only
    // writes that word.  Launch latency, the gap between two launches of one stream, the index draw and the weight staging then run
    // under step t and the host's turn (kernels.h: DqnStepArgs::go_flag).  FRL_ROLLOUT_PREARM=0/1 overrides.
    const bool forced = knob_flag(k.prearm, false), allowed = knob_flag(k.prearm, true);
    // (a solo engine's launches need every workgroup resident — the flag hand-overs spin — so an armed launch must fit NEXT to the running
    // one whatever the switch says: 2 x 16 workgroups per learner on the device's CUs (frl_engine::n_cus); past that the armed workgroups would hold the CUs the
    // running step's actor launch is waiting for, until their 2 s bound)
    const bool fits = pl.fold == FOLD_DQN || (long long)f.P * 2 * std::max(f.solo, 1) <= f.n_cus;
    // (defaults from tools/prearm_soak.py, us per vector step armed / plain: DQN with 8 / 16 / 32 learners 23.8 / 33.1, 27.3 / 34.4, 33.6 / 36.3;
    // TD3 on the solo kernels with 4 / 8 learners 80.9 / 78.4, 100.6 / 89.2 — their armed workgroups' polling costs more than it hides)
    pl.prearm = ((pl.fold == FOLD_DQN && f.P <= 32) || (pl.fold == FOLD_SOLO && f.P <= 2) || forced) && pl.fold != FOLD_NONE && fits && pl.poll &&
                !f.profile && allowed;
    // A pre-armed launch gives up after 2 s of spinning (a bound on what a stuck host can do to the GPU).  An env whose step takes that
    // long must not lose its update to that: past arm_patience between arming and the doorbell the host CANCELS the launch for certain
    // (-1 in the doorbell, both streams drained — a launch that gives up has touched nothing), puts every counter the arming advanced
    // back, and the caller launches the step the plain way with the same arguments.  FRL_ROLLOUT_ARM_PATIENCE_MS: the bound in
    // milliseconds (tests: 0 = every armed launch is cancelled and replayed).
    pl.arm_patience = k.arm_patience_ms * 1e-3;
    pl.timing = k.timing;
    *out = pl;
    return FRL_OK;
}

// Is vector step `step` (0-based) a learn step, the smallest ring holding min_size rows once its rows are in?  The one predicate: the
// loop asks it for the step it is in, and — with step + 1 and the predicted size — for the step it arms a launch for.
inline bool learn_due(const frl_rollout_args& ra, int step, int min_size) {
    return ra.learn_every > 0 && (step + 1) % ra.learn_every == 0 && min_size > ra.start_steps && min_size >= 2 * ra.learn.batch;
}

// The one block a vector step uploads (or the launch reads in place), sections 16-byte aligned:
// [scale P f32 | row n i32 | next_obs n*O | obs_next n*O | reward n | flags n u8]
struct BlkView { float* scale; int* row; float* next_obs; float* obs_next; float* reward; unsigned char* flags; };
struct BlkLayout {
    size_t off_row = 0, off_nobs = 0, off_onext = 0, off_rew = 0, off_flags = 0, bytes = 0;
    BlkLayout() = default;
    BlkLayout(size_t P, size_t n, size_t O) {
        auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
        off_row = up16(P * sizeof(float));
        off_nobs = up16(off_row + n * sizeof(int));
        off_onext = up16(off_nobs + n * O * sizeof(float));
        off_rew = up16(off_onext + n * O * sizeof(float));
        off_flags = up16(off_rew + n * sizeof(float));
        bytes = up16(off_flags + n);
    }
    // the sections from any base: the pinned host block, its upload, or the host block's device-visible alias
    BlkView view(unsigned char* base) const {
        return {(float*)base, (int*)(base + off_row), (float*)(base + off_nobs), (float*)(base + off_onext), (float*)(base + off_rew), base + off_flags};
    }
};

}  // namespace frl
