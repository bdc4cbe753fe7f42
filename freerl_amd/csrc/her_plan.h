// Hindsight relabelling of ONE finished episode inside a learner's replay ring (DDPG_file/DDPG_simple_try_HER.py:267-279,421-428):
// how many relabelled rows follow each transition, where they go, which ring rows they read, and the one rule set that refuses a call.
// Plain C++17 without HIP: frl_her_relabel (frl_api_her.inc) validates and advances the cursors through it, her_relabel_kernel
// (kernels_her.hip) addresses through it, tests/her_plan_probe.cpp walks it on the CPU.  Nothing else may compute these.
//
// The episode's L real rows are the L rows behind the cursor: transition i sits in ring row src(i) = (start + i) % capacity with
// start = (cursor - L) mod capacity.  Transition i is followed by n_i = min(sample_num, sample_range, L - i) relabelled rows (the
// candidates are transitions i .. i + m_i - 1, m_i = min(sample_range, L - i)); output ordinal r = prefix(i) + s, s in [0, n_i), goes
// to ring row dst(r) = (cursor + r) % capacity.  L + total <= capacity keeps every destination row off every source row.
#pragma once

#if defined(__HIPCC__)
#define FRL_HER_HD __host__ __device__
#else
#define FRL_HER_HD
#endif

namespace frl {

constexpr int kHerMaxSamples = 8;        // sample_num: the relabelled rows one transition may be followed by

// with q = min(sample_num, sample_range): n_i = q for the first T = max(0, L - q + 1) transitions, L - i for the tail
struct HerPlan {
    int capacity, cursor, L, q, range, T;
};

FRL_HER_HD inline HerPlan her_plan(int capacity, int cursor, int L, int sample_num, int sample_range) {
    HerPlan p;
    p.capacity = capacity; p.cursor = cursor; p.L = L;
    p.q = sample_num < sample_range ? sample_num : sample_range;
    p.range = sample_range;
    p.T = L - p.q + 1 > 0 ? L - p.q + 1 : 0;
    return p;
}

// candidates of transition i (step i itself among them), and how many of them are used
FRL_HER_HD inline int her_m(const HerPlan& p, int i) { return p.range < p.L - i ? p.range : p.L - i; }
FRL_HER_HD inline int her_n(const HerPlan& p, int i) { return p.q < p.L - i ? p.q : p.L - i; }

// output ordinal of transition i's first relabelled row; i == L: the episode's total
FRL_HER_HD inline long long her_prefix(const HerPlan& p, int i) {
    if (i <= p.T) return (long long)i * p.q;
    const long long t = i - p.T;                      // tail transitions T .. i-1 give L - T, L - T - 1, ...
    return (long long)p.T * p.q + t * p.L - ((long long)p.T + i - 1) * t / 2;
}
FRL_HER_HD inline long long her_total(const HerPlan& p) { return her_prefix(p, p.L); }

// the inverse: output ordinal r in [0, total) -> transition i and its slot s in [0, n_i)
FRL_HER_HD inline void her_locate(const HerPlan& p, long long r, int& i, int& s) {
    const long long head = (long long)p.T * p.q;
    if (r < head) { i = (int)(r / p.q); s = (int)(r - (long long)i * p.q); return; }
    r -= head;
    i = p.T;
    while (r >= p.L - i) { r -= p.L - i; ++i; }       // at most q - 1 <= 7 steps
    s = (int)r;
}

FRL_HER_HD inline int her_start(const HerPlan& p) { return ((p.cursor - p.L) % p.capacity + p.capacity) % p.capacity; }
FRL_HER_HD inline int her_src(const HerPlan& p, int i) { return (int)(((long long)her_start(p) + i) % p.capacity); }
FRL_HER_HD inline int her_dst(const HerPlan& p, long long r) { return (int)(((long long)p.cursor + r) % p.capacity); }

// ---- the refusal rules, in the order they are judged (the first that fails names the refusal)
enum HerRefusal : int {
    HER_OK = 0,
    HER_BAD_SAMPLE_NUM,      // 1 <= sample_num <= kHerMaxSamples
    HER_BAD_SAMPLE_RANGE,    // sample_range >= 1
    HER_BAD_GOAL_DIM,        // 1 <= goal_dim <= state_dim
    HER_BAD_OBS_DIM,         // state_dim + goal_dim == the engine's obs_dim
    HER_EMPTY_EPISODE,       // L >= 1
    HER_EPISODE_NOT_STORED,  // L <= the learner's stored rows
    HER_NO_ROOM              // L + total <= capacity
};

struct HerShape {            // what does not depend on the episode
    int obs_dim, state_dim, goal_dim, sample_num, sample_range;
};

inline HerRefusal her_check_shape(const HerShape& s) {
    if (s.sample_num < 1 || s.sample_num > kHerMaxSamples) return HER_BAD_SAMPLE_NUM;
    if (s.sample_range < 1) return HER_BAD_SAMPLE_RANGE;
    if (s.goal_dim < 1 || s.goal_dim > s.state_dim) return HER_BAD_GOAL_DIM;
    if ((long long)s.state_dim + s.goal_dim != s.obs_dim) return HER_BAD_OBS_DIM;
    return HER_OK;
}

inline HerRefusal her_check_episode(const HerShape& s, int capacity, int size, int L) {
    if (L < 1) return HER_EMPTY_EPISODE;
    if (L > size) return HER_EPISODE_NOT_STORED;
    if (L + her_total(her_plan(capacity, 0, L, s.sample_num, s.sample_range)) > capacity) return HER_NO_ROOM;
    return HER_OK;
}

inline HerRefusal her_check(const HerShape& s, int capacity, int size, int L) {
    const HerRefusal r = her_check_shape(s);
    return r != HER_OK ? r : her_check_episode(s, capacity, size, L);
}

inline const char* her_refusal_text(HerRefusal r) {
    switch (r) {
        case HER_OK: return "ok";
        case HER_BAD_SAMPLE_NUM: return "sample_num outside [1, 8]";
        case HER_BAD_SAMPLE_RANGE: return "sample_range below 1";
        case HER_BAD_GOAL_DIM: return "goal_dim outside [1, state_dim]";
        case HER_BAD_OBS_DIM: return "state_dim + goal_dim is not the engine's obs_dim";
        case HER_EMPTY_EPISODE: return "an episode of no steps";
        case HER_EPISODE_NOT_STORED: return "the episode is longer than the learner's stored rows";
        case HER_NO_ROOM: return "the episode and its relabelled rows do not fit the ring (L + total > capacity)";
    }
    return "?";
}

}  // namespace frl
