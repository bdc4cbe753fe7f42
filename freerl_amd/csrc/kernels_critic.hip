// Critic gradient kernel of DDPG / TD3 / SAC / MADDPG / MATD3 (see kernels_update.hip for the launch chain).
#include <hip/hip_runtime.h>

#include "device/net.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// ------------------------------------------------------- DDPG / TD3 / SAC / MADDPG: critic
// TD target with the target nets, twin/single critic forward, MSE delta, backward -> slab.
// DDPG_simple.py:139-149, TD3.py:193-213, SAC.py:226-238, MADDPG_simple.py:169-176.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void ac_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = agent_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int n = D.n_agents, p = U.p, ag = U.ag;
    const RecordDesc& R = D.rec;
    const NetDesc& NC = D.net[2 * ag + 1];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.batch;
    const RowWalk W = U.walk(B);
    const bool sac = (D.algo == ALGO_SAC);
    g_cf thC = U.theta(2 * ag + 1);
    g_cf tgC = U.target(2 * ag + 1);
    g_f slab = U.slab(2 * ag + 1);
    g_cf ring = U.ring();
    const int am = D.act_max;
    const int OT = R.obs_total, AT = R.act_total, kc0 = NC.L[0].k_pad;
    const float alpha = sac ? D.alpha[p * 4 + 3] : 0.f;
    const float invB = 1.f / (float)B;
    const bool direct = (n == 1) && kc0 <= D.net[0].L[0].k_pad;      // a' can be written into the critic input in place
    // Batch_ObsNorm statistics as of THIS agent's sample() (version ag), one block of obsnorm_w per agent
    g_cf bn = D.obs_norm_on ? as_global(D.obsnorm + ((size_t)p * n + ag) * n * D.obsnorm_w) : nullptr;
    auto normalize_joint = [&](int nvalid) {      // every agent's segment of a joint [obs_0 | obs_1 | ...] block in xin[:, 0:OT)
        for (int j = 0; j < n; ++j)
            normalize_cols(S.xin, S.xp, nvalid, R.obs_off[j] - R.obs_off[0], R.obs_dim[j], bn + (size_t)j * D.obsnorm_w, R.obs_dim[j]);
    };
    FRL_PHASE_INIT(S);

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int nv = c.nv;
    g_ci idx = c.idx;
    g_cf noise_u = c.noise;
    // ---- a' = actor_target_j(s'_j) for every agent j (MADDPG_simple.py:155; n = 1 otherwise)
    float lp_next = 0.f;                            // SAC: log pi(a'|s') of row threadIdx.x
    for (int j = 0; j < n; ++j) {
        const NetDesc& NJ = D.net[2 * j];
        g_cf tgJ = U.target(2 * j);
        const int Oj = R.obs_dim[j], Aj = R.act_dim[j], cj = R.act_off[j] - R.act_off[0];
        g_cf noise0 = noise_u + (size_t)j * D.batch_max * am;     // set j (n = 1: set 0); MATD3_simple.py:199-201
        gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[j], Oj, 0);
        zero_cols(S.xin, S.xp, rc, Oj, NJ.L[0].k_pad);
        if (bn) { lds_barrier(); normalize_cols(S.xin, S.xp, nv, 0, Oj, bn + (size_t)j * D.obsnorm_w, Oj); }
        FRL_PHASE(S);
        // a'_j per row in the finalize phase of the target actor; single agent: straight into the critic's input row
        // (xin[:, 0:O) still holds the normalised next_obs, the columns past the action are already zero)
        mlp_fwd_rows(NJ, 0, NJ.n_layers, tgJ, S, sac ? ACT_NONE : ACT_TANH, [&](int r) {
            if (sac) {                              // SAC.py:70-97 on actor_target (SAC.py:227)
                float lp = 0.f;
                for (int c = 0; c < Aj; ++c) {
                    const float eps = (r < nv) ? noise0[(size_t)r * am + c] : 0.f;
                    S.abuf[r * S.ap + cj + c] = sac_sample(S.outb[r * S.op + c], tgJ[NJ.extra_off + c], eps, lp);
                }
                lp_next = lp;
            } else {
                for (int c = 0; c < Aj; ++c) {
                    float v = S.outb[r * S.op + c];
                    if (a.use_policy_noise && r < nv) v = td3_smooth(a, v, noise0[(size_t)r * am + c]);
                    S.abuf[r * S.ap + cj + c] = v;
                }
            }
            if (direct)
                for (int c = 0; c < Aj; ++c) S.xin[r * S.xp + OT + c] = S.abuf[r * S.ap + c];
        });
    }
    // ---- centralised target critic on [next_obs_all | a'_all]
    // single agent: xin[:, 0:O) still holds the (normalised) next_obs the target actor has just read
    if (!direct) {
        if (n > 1) gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], OT, 0);
        joint_actions_to_xin(S, OT, AT, kc0);
        if (bn && n > 1) { lds_barrier(); normalize_joint(nv); }
        FRL_PHASE(S);
    }
    const float q = target_q_min(NC, tgC, S);
    if (threadIdx.x < nv) {
        g_cf rec = ring + (size_t)idx[threadIdx.x] * R.stride;
        const float rew = rec[R.rew_off + ag], done = rec[R.done_off + ag];
        S.y[threadIdx.x] = sac ? td_target_sac(rew, done, a.gamma, q, alpha, lp_next) : td_target(rew, done, a.gamma, q);
    }
    FRL_PHASE(S);

    // ---- critic heads on the stored [obs | act] rows: forward, TD delta, backward
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], OT + AT, 0);
    zero_cols(S.xin, S.xp, rc, OT + AT, kc0);
    if (bn) { lds_barrier(); normalize_joint(nv); }
    critic_heads_td(NC, thC, slab, S, a, nv, c.gs, invB, lossp);
    }
    FRL_PHASE_DUMP(S, 0);
    store_loss_part(U, S, lossp);
}
}  // namespace frl
