// What an on-policy learn call (frl_ppo_learn, frl_gail_ppo_learn, frl_mappo_learn, frl_happo_learn) decides before it touches the
// device: which calls are refused, where the minibatch permutations come from, where every array of the d_ppo / d_perm scratch lies
// and how large the two are, and the host's own draws.  Plain C++17, no HIP, no getenv, so tests/onpolicy_plan_probe.cpp walks every
// rule on the CPU (tests/test_onpolicy_plan.py).  The three frl_api_*ppo.inc files plan, grow the scratch to the layout's totals and launch.
#pragma once
#include "engine_plan.hpp"

namespace frl {

enum OnpolicyFamily { ONP_PPO, ONP_GAIL_PPO, ONP_MAPPO };      // (ONP_MAPPO: frl_mappo_learn and frl_happo_learn)
// the caller's np.random.permutation / torch.randperm draws; ppo_perm_kernel (a sort of random keys per unit and epoch, Tpad keys in
// LDS); past 8192 rows a Fisher-Yates on the host
enum PermSource { PERM_CALLER, PERM_DEVICE, PERM_HOST };

// units: what draws its own permutations — a learner, for MAPPO / HAPPO a (learner, agent)
struct OnpolicyCall {
    int T = 0, mb = 0, K = 0, n_mb = 0, Tpad = 2;
    size_t units = 0;
    PermSource perms = PERM_DEVICE;
    size_t rows() const { return units * (size_t)T; }                   // floats of one [units][T] array
    size_t perm_n() const { return units * (size_t)K * T; }             // [units][K][T]
    size_t trace_n() const { return units * (size_t)K * n_mb * 2; }     // (actor, critic) loss of every minibatch step
};

// FRL_OK and *out, or FRL_ERR_INVALID and *message
inline int plan_onpolicy(OnpolicyFamily fam, int capacity, int batch_max, size_t units, int T, int mb, int K, bool caller_perms,
                         OnpolicyCall* out, std::string* message) {
    if (fam == ONP_GAIL_PPO) {
        if (T < 2) return plan_refuse(message, "horizon %d < 2: the unbiased std of one advantage is NaN", T);
        if (T > capacity) return plan_refuse(message, "horizon %d > capacity %d", T, capacity);
    } else if (T < 2 || T > capacity) {
        return plan_refuse(message, "horizon %d outside [2, capacity %d]", T, capacity);
    }
    if (mb < 1 || mb > batch_max) return plan_refuse(message, "minibatch %d outside [1,%d]", mb, batch_max);
    if (K < 1) return plan_refuse(message, "k_epochs must be >= 1");
    OnpolicyCall c;
    c.T = T; c.mb = mb; c.K = K; c.units = units;
    c.n_mb = (T + mb - 1) / mb;
    while (c.Tpad < T) c.Tpad <<= 1;
    c.perms = caller_perms ? PERM_CALLER : c.Tpad <= 8192 ? PERM_DEVICE : PERM_HOST;
    *out = c;
    return FRL_OK;
}

// The scratch of a call: offsets in floats from d_ppo, taken in ONE pass, so that the total mem.grow is asked for is where the pass ended
struct Carve {
    size_t at = 0;
    size_t take(size_t n) { const size_t o = at; at += n; return o; }
};
struct PpoLayout { size_t td, vs, adv_raw, adv, vtarget, trace, floats, ints; };
inline PpoLayout ppo_layout(const OnpolicyCall& c) {
    Carve q;
    PpoLayout L;
    L.td = q.take(c.rows()); L.vs = q.take(c.rows()); L.adv_raw = q.take(c.rows()); L.adv = q.take(c.rows()); L.vtarget = q.take(c.rows());
    L.trace = q.take(c.trace_n());
    L.floats = q.at; L.ints = c.perm_n();
    return L;
}
struct GailPpoLayout { size_t vs, logp_old, td, adv_raw, adv, returns, rewards, last_value, trace, floats, ints; };
inline GailPpoLayout gail_ppo_layout(const OnpolicyCall& c) {
    Carve q;
    GailPpoLayout L;
    L.vs = q.take(c.rows()); L.logp_old = q.take(c.rows()); L.td = q.take(c.rows()); L.adv_raw = q.take(c.rows()); L.adv = q.take(c.rows());
    L.returns = q.take(c.rows()); L.rewards = q.take(c.rows());
    L.last_value = q.take(c.units);
    L.trace = q.take(c.trace_n());
    L.floats = q.at; L.ints = c.perm_n();
    return L;
}
// happo: old [P][T] and factor [P][n][T] behind the trace, the visiting order [P][n] (ints from d_perm) behind the permutations
struct MappoLayout { size_t td, advd, vs, adv_seq, adv_raw, adv, vtarget, trace, old, factor, floats, order, ints; };
inline MappoLayout mappo_layout(const OnpolicyCall& c, size_t P, bool happo) {
    Carve q, qi;
    MappoLayout L;
    L.td = q.take(c.rows()); L.advd = q.take(c.rows()); L.vs = q.take(c.rows()); L.adv_seq = q.take(c.rows()); L.adv_raw = q.take(c.rows());
    L.adv = q.take(c.rows()); L.vtarget = q.take(c.rows());
    L.trace = q.take(c.trace_n());
    L.old = q.take(happo ? P * c.T : 0); L.factor = q.take(happo ? c.rows() : 0);
    qi.take(c.perm_n());
    L.order = qi.take(happo ? c.units : 0);
    L.floats = q.at; L.ints = qi.at;
    return L;
}

// A caller's int64 draws, range-checked and narrowed
inline int narrow_perms(const int64_t* perms, size_t n, int T, std::vector<int>* out, std::string* message) {
    out->resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (perms[i] < 0 || perms[i] >= T) return plan_refuse(message, "permutation entry %lld outside [0,%d)", (long long)perms[i], T);
        (*out)[i] = (int)perms[i];
    }
    return FRL_OK;
}

inline unsigned long long splitmix64(unsigned long long& s) {
    unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// `blocks` Fisher-Yates shuffles of 0..len-1 from one splitmix64 stream keyed by the engine's seed and the call's rng_counter value
inline void host_shuffle(unsigned long long seed, unsigned long long counter, size_t blocks, int len, std::vector<int>* out) {
    out->resize(blocks * len);
    unsigned long long s = seed ^ (0xD1B54A32D192ED03ull * counter);
    for (size_t blk = 0; blk < blocks; ++blk) {
        int* q = out->data() + blk * len;
        for (int i = 0; i < len; ++i) q[i] = i;
        for (int i = len - 1; i > 0; --i) std::swap(q[i], q[(int)(splitmix64(s) % (unsigned long long)(i + 1))]);
    }
}

}  // namespace frl
