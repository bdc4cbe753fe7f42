// Hindsight experience replay (DDPG_file/DDPG_simple_try_HER.py:267-286,421-428): when an episode ends, every transition i is stored
// again up to sample_num times with the goal replaced by the achieved goal of a transition j >= i of the same episode ("future").
// The relabelled rows are pure functions of rows that already sit in the GPU-resident ring, so one launch writes them where they live,
// for every learner whose episode ended: no host loop of policy.add calls, nothing through pinned staging.  Byte work, no LDS.
//
// Record: obs = [state (S) | goal (G)], achieved goal = next state[0:G].  Relabelled row of (i, j):
//   obs = [state_i | g], action = the env action of step i (or the stored one), reward = calcu_reward(g, state_i), next_obs =
//   [next_state_i | g], done = 0, with g = next_state_j[0:G].
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/rng.hpp"
#include "frl_desc.h"
#include "her_plan.h"

namespace frl {

// calcu_reward (:247-265): cost = sum_c w_c (g_c - s_c)^2 accumulated in float64 left to right from the stored float32 values, every
// product and sum rounded on its own (no fused multiply-add: the script's Python arithmetic has none).
__device__ __forceinline__ float her_reward(const float* __restrict__ state, const float* __restrict__ goal, const HerArgs& a) {
#pragma clang fp contract(off)
    double cost = 0.0;
    for (int c = 0; c < a.G; ++c) {
        const double d = (double)goal[c] - (double)state[c];
        const double sq = d * d;
        const double t = a.weights[c] * sq;
        cost = c == 0 ? t : cost + t;
    }
    if (a.mode == 1) return (float)(-cost);
    return cost < a.tolerance ? 0.f : -1.f;
}

// random.sample(candidates, k) as a set (:278): k distinct offsets in [0, m), uniform over the k-subsets, by Floyd's algorithm — draw
// t picks x in [0, m - k + t]; x if it is new, else m - k + t.  k draws, no table; every lane group of a transition repeats them and
// keeps slot s.  Keyed by (relabel call, learner, transition, draw).
__device__ __forceinline__ int her_draw(const HerArgs& a, int learner, int i, int m, int k, int s) {
    int chosen[kHerMaxSamples], out = 0;
    const unsigned long long key = a.seed ^ 0x48696E6473696768ull;
#pragma unroll
    for (int t = 0; t < kHerMaxSamples; ++t) {
        chosen[t] = -1;
        if (t < k) {
            const int top = m - k + t;
            int x = (int)uniform_index(philox4x32_10(a.counter, (unsigned)learner, (unsigned)i * kHerMaxSamples + t, key), (unsigned)top + 1u);
            bool seen = false;
#pragma unroll
            for (int u = 0; u < t; ++u) seen |= chosen[u] == x;
            chosen[t] = seen ? top : x;
            if (t == s) out = chosen[t];
        }
    }
    return out;
}

// A 16-lane group owns one relabelled row: (episode blockIdx.y, output ordinal r).  Source and picked rows are read, the destination
// row is written; the plan keeps destination rows off source rows, and the episodes of a call belong to different learners.
__global__ void her_relabel_kernel(float* __restrict__ ring, RecordDesc rec, HerArgs a) {
    const int* ep = a.eps + (size_t)blockIdx.y * HER_EP_INTS;
    const int learner = ep[HER_EP_LEARNER];
    const HerPlan pl = her_plan(a.capacity, ep[HER_EP_CURSOR], ep[HER_EP_L], a.sample_num, a.sample_range);
    const long long r = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int lane = threadIdx.x & 15;
    if (r >= her_total(pl)) return;
    int i, s;
    her_locate(pl, r, i, s);
    const int m = her_m(pl, i), n = her_n(pl, i);
    int o = s;                                                   // m < sample_num: every candidate, in order
    if (a.picks) o = a.picks[(size_t)ep[HER_EP_PICK0] + r];
    else if (m >= a.sample_num) o = her_draw(a, learner, i, m, n, s);
    o = o < 0 ? 0 : (o >= m ? m - 1 : o);                        // (the host refuses injected picks outside [0, m))
    float* base = ring + (size_t)learner * a.capacity * rec.stride;
    const float* src = base + (size_t)her_src(pl, i) * rec.stride;
    const float* pick = base + (size_t)her_src(pl, i + o) * rec.stride;
    float* dst = base + (size_t)her_dst(pl, r) * rec.stride;
    const int oo = rec.obs_off[0], no = rec.nobs_off[0];
    for (int c = lane; c < a.S; c += 16) {
        dst[oo + c] = src[oo + c];
        dst[no + c] = src[no + c];
    }
    for (int c = lane; c < a.G; c += 16) {
        const float g = pick[no + c];
        dst[oo + a.S + c] = g;
        dst[no + a.S + c] = g;
    }
    const float* act = a.env_actions ? a.env_actions + ((size_t)ep[HER_EP_ACT0] + i) * a.A : src + rec.act_off[0];
    for (int c = lane; c < a.A; c += 16) dst[rec.act_off[0] + c] = act[c];
    for (int c = lane; c < rec.extra; c += 16) dst[rec.extra_off + c] = 0.f;      // what Buffer.add leaves there
    if (lane == 0) {
        dst[rec.rew_off] = her_reward(src + oo, pick + no, a);
        dst[rec.done_off] = 0.f;
    }
}

}  // namespace frl
