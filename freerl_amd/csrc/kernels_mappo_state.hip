// MAPPO with a global-state critic (MAPPO_file/MAPPO_for_mask_action_state.py:122-156, 310-323, 371-373) on a FRL_ALGO_MAPPO engine
// created through frl_create_ex with state_dim > 0: the last state_dim columns of a record's extra block hold env.get_state()
// (EngineDesc::state_off) and every critic's first layer is obs_total + state_dim columns wide.  One learn() is
//     mappo_state_values_kernel -> gae_dense_kernel -> mappo_adv_kernel -> mappo_state_update_kernel | mappo_state_mask_update_kernel
// The value pass is mappo_values_kernel with the critic's row filled from two segments, the update is mappo_update_kernel's /
// mappo_mask_update_kernel's grid and step loop (device/mappo.hpp: mappo_steps) with kState set: only the critic's row differs.  The
// actors, select_action (mappo_act_kernel, mappo_mask_act_kernel), the GAE scan and the advantages do not see the state.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/act_common.hpp"
#include "device/mappo.hpp"

namespace frl {

// ---- td_delta_i = r_i + gamma (1 - done_i) V_i(s') - V_i(s) with V(s) = critic([obs(t) | state(t)]) and V(s') = critic([next_obs(t) |
// state(t)]): the SAME state row in both (:322-323), not a next state; grid (chunks, P * n)
__global__ __launch_bounds__(256) void mappo_state_values_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, u = blockIdx.y, p = u / n, i = u - p * n;
    const int rc = D.rc, r0 = blockIdx.x * rc, T = a.horizon, nv = min(rc, T - r0);
    const NetDesc& N = D.net[2 * i + 1];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    g_cf theta = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[2 * i + 1]);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    const CriticIn ci = critic_in(D, i);
    const int kpad = N.L[0].k_pad, ow = ci.width, kin = ow + D.state_dim;
    float v0 = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        const int src = pass == 0 ? ci.obs : ci.nobs;
        for (int e = threadIdx.x; e < rc * kpad; e += kWG) {
            const int r = e / kpad, c = e - r * kpad;
            float x = 0.f;
            if (r < nv && c < kin) x = ring[(size_t)(r0 + r) * R.stride + (c < ow ? src + c : D.state_off + (c - ow))];
            S.xin[r * S.xp + c] = x;
        }
        __syncthreads();
        mappo_fwd(D, N, theta, S, X, kin, ACT_NONE);
        if (threadIdx.x < nv) {
            const float v = S.outb[threadIdx.x * S.op];
            if (pass == 0) {
                v0 = v;
            } else {
                g_cf rec = ring + (size_t)(r0 + threadIdx.x) * R.stride;
                const size_t o = (size_t)u * T + r0 + threadIdx.x;
                a.vs[o] = v0;
                a.td[o] = rec[R.rew_off + i] + a.gamma * (1.f - rec[R.done_off + i]) * v - v0;
                a.advd[o] = rec[R.extra_off + R.act_total + i];
            }
        }
        __syncthreads();
    }
}

// ---- all minibatch steps of one net of one (learner, agent); grid (P * n, 2): blockIdx.y 0 = the actor's steps, 1 = the critic's.
// Continuous actors, or discrete actors without masks (EngineDesc::mask_off 0)
__global__ __launch_bounds__(256) void mappo_state_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x / D.n_agents, i = blockIdx.x - p * D.n_agents;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    mappo_steps<false, false, true>(D, a, S, carve_mappo(S), p, i, blockIdx.y == 0, nullptr);
}

// ---- the same with the discrete actors' rows under their mask blocks (EngineDesc::mask_off set)
__global__ __launch_bounds__(256) void mappo_state_mask_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x / D.n_agents, i = blockIdx.x - p * D.n_agents;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    mappo_steps<false, true, true>(D, a, S, carve_mappo(S), p, i, blockIdx.y == 0, nullptr);
}

}  // namespace frl
