// MAPPO with invalid-action masking (MAPPO_file/MAPPO_for_mask_action.py:191-215, 245-264, 299-387) on a FRL_ALGO_MAPPO engine whose
// records carry one mask block per agent behind the adv_done columns (EngineDesc::mask_off, frl_action_mask_set).  One learn() is
//     mappo_values_kernel -> gae_dense_kernel -> mappo_adv_kernel -> mappo_mask_update_kernel
// the first three as kernels_mappo.hip has them: the critic, the GAE scan and the advantages do not see the masks.  The update is
// mappo_update_kernel's grid and step loop (device/mappo.hpp: mappo_steps) with the discrete actor's row read as CategoricalMasked
// (device/onpolicy.hpp: masked_cat_row); select_action's draw is mappo_mask_act_kernel, on the same row arithmetic.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/act_common.hpp"
#include "device/mappo.hpp"

namespace frl {

// ---- all minibatch steps of one net of one (learner, agent); grid (P * n, 2): blockIdx.y 0 = the actor's steps, 1 = the critic's
__global__ __launch_bounds__(256) void mappo_mask_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x / D.n_agents, i = blockIdx.x - p * D.n_agents;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    mappo_steps<false, true>(D, a, S, carve_mappo(S), p, i, blockIdx.y == 0, nullptr);
}

// ---- frl_act_masked: CategoricalMasked(logits = actor(obs), masks).sample() and its log_prob for n_rows rows per learner; grid
// (chunks, P).  mask [P][n_rows][out_dim], nonzero = available.  The draw is torch's single-draw multinomial, argmax(p_c / q_c) with
// q ~ Exp(1) injected (a.eps) or from the launch's Philox stream; a closed action has p = 0 and cannot win while one is open (a row
// with none open has p = 1 / A in every column).  The log-prob is the drawn column's normalised logit, not clamped.
__global__ __launch_bounds__(256) void mappo_mask_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a, const float* __restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc;
    const NetDesc& N = D.net[a.net];
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    const int rc = D.rc, nv = min(rc, a.n_rows - r0);
    g_cf theta = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[a.net]);
    const int K = a.in_dim, kpad = N.L[0].k_pad, A = N.L[2].n;
    g_cf in = as_global(a.in + ((size_t)p * a.n_rows + r0) * K);
    load_rows(S.xin, S.xp, rc, nv, in, 0, K, 0, K, kpad);
    __syncthreads();
    mappo_fwd(D, N, theta, S, X, K, ACT_NONE);
    const unsigned long long key = D.seed + 0x9E3779B97F4A7C15ull * (p + 1);      // act_epilogue's key: (seed, learner), one counter per launch
    for (int r = threadIdx.x; r < nv; r += kWG) {
        const size_t row = (size_t)p * a.n_rows + r0 + r;
        lds_cf z = S.outb + r * S.op;
        const MaskedCatRow q = masked_cat_row(z, as_global(mask + row * A), A);
        int best = 0;
        float bestv = -1.f, lbest = 0.f;
        for (int c = 0; c < A; ++c) {
            const float l = q.logit(z[c], c);
            const float qc = a.device_eps ? -logf(u01(philox4x32_10(a.rng_counter, 0x9100u, (unsigned)((r0 + r) * A + c), key).x)) : a.eps[row * A + c];
            const float v = q.prob(l) / qc;
            if (v > bestv) { bestv = v; best = c; lbest = l; }
        }
        a.out[row] = (float)best;
        if (a.out_logp) a.out_logp[row] = lbest;
    }
}

}  // namespace frl
