// HAPPO (MAPPO_file/HAPPO.py:339-458): MAPPO's nets, ring, value pass, GAE scan and advantage launch, but the agents are visited in a
// random order and a later agent's surrogate is weighted, row by row, with the product of the earlier agents' new-over-old policy
// ratios over the whole horizon (:373-376, :415, :443-453).  One learn() is
//     mappo_values_kernel -> gae_dense_kernel -> mappo_adv_kernel -> happo_update_kernel x n_agents (one per visiting position)
// The dependency between agents is carried by stream order between the launches and by nothing else: launch k reads factor slice k,
// which launch k-1 finished writing, and writes slice k+1; no workgroup reads what another workgroup of its own launch writes.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/act_common.hpp"
#include "device/mappo.hpp"

namespace frl {

// sum_c log pi(a_t | o_t) of agent i's actor as it stands, rows 0..T-1 in time order (HAPPO.py:382-391, :443-452; the discrete branch
// over all rows too: DESIGN.md "HAPPO").  first: old[t] = that; else next[t] = cur[t] * exp(that - old[t]) (cur == nullptr: ones).
// Row t belongs to thread t % rc in both passes, so old[] is read by the thread that wrote it.
__device__ __forceinline__ void happo_horizon_pass(const EngineDesc& D, const Lds& S, const MappoLds& X, int p, int i, int T, bool first, g_f old,
                                                   g_cf cur, g_f next) {
    const NetDesc& N = D.net[2 * i];
    const RecordDesc& R = D.rec;
    g_cf th = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[2 * i]);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    const bool discrete = D.n_discrete > 0;
    const int rc = D.rc, O = R.obs_dim[i], A = N.L[2].n, kpad = N.L[0].k_pad;
    for (int r0 = 0; r0 < T; r0 += rc) {
        const int nv = min(rc, T - r0);
        load_rows(S.xin, S.xp, rc, nv, ring, r0, R.stride, R.obs_off[i], O, kpad);
        __syncthreads();
        mappo_fwd(D, N, th, S, X, O, discrete ? ACT_NONE : ACT_TANH);
        if (threadIdx.x < nv) {
            const int r = threadIdx.x, t = r0 + r;
            g_cf rec = ring + (size_t)t * R.stride;
            lds_cf z = S.outb + r * S.op;
            const float lp = discrete ? cat_row(z, A).logp_at(z, A, (int)rec[R.act_off[i]])
                                      : normal_row_logp(rec + R.act_off[i], z, th + N.extra_off, A, kLogStdMin, kLogStdMax);
            if (first) old[t] = lp;
            else next[t] = (cur ? cur[t] : 1.f) * expf(lp - old[t]);
        }
        __syncthreads();
    }
}

// ---- visiting position x.k of every learner; grid (P, 2): blockIdx.y 0 = all actor steps of the visited agent i = order[p][k] between
// its two horizon passes, 1 = all steps of that agent's critic (the reference's pairing, HAPPO.py:416-440; a critic reads no actor)
__global__ __launch_bounds__(256) void happo_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a, HappoArgs x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, p = blockIdx.x, T = a.horizon, k = x.k;
    const int i = x.order[p * n + k];
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    if (blockIdx.y == 1) {
        mappo_steps<false>(D, a, S, X, p, i, false, nullptr);
        return;
    }
    g_f fac = as_global(x.factor + (size_t)p * n * T);
    g_f old = as_global(x.old + (size_t)p * T);
    g_cf cur = k ? fac + (size_t)k * T : nullptr;            // position 0: the factor is 1 and is not read
    if (k == 0)
        for (int t = threadIdx.x; t < T; t += kWG) fac[t] = 1.f;       // (slice 0 is written for frl_happo_args::factor_out only)
    const bool more = k < n - 1;
    if (more) happo_horizon_pass(D, S, X, p, i, T, true, old, nullptr, nullptr);
    mappo_steps<true>(D, a, S, X, p, i, true, cur);
    if (more) happo_horizon_pass(D, S, X, p, i, T, false, old, cur, fac + (size_t)(k + 1) * T);
}

}  // namespace frl
