// MASAC (MAAC_file/MASAC.py:219-277; entropy_way_c = entropy_way_a = action_way = '1', adaptive alpha): the gradient kernels of an
// ALGO_MASAC engine and the stacked head's forward for frl_act.  The row-chunk skeleton of kernels_critic.hip / kernels_actor.hip — a
// workgroup walks `cps` chunks of rc rows and leaves one gradient slab; reduce + clip + Adam, the alpha step and the soft updates are
// kernels_update.hip's — around what MASAC does differently from SAC and MATD3:
//   * the actor's head is [mean | log_std], 2 A columns: log_std is a head column of the row, clamped per row;
//   * the TD target samples EVERY agent's target actor and keeps the updating agent's log-prob and alpha only;
//   * the actor loss sends the fresh actions of ALL n online actors through the agent's own twin critic and takes the minimum per row;
//   * its entropy is a second, independent draw of the agent's own actor;
//   * the actor launch is for ONE agent (LearnArgs::agent): agent i reads the online actors of agents j < i as they have just stepped.
// Draw sets of D.noise, per updating agent: j = target actor j, n + j = online actor j, 2 n = the entropy draw.
#include <hip/hip_runtime.h>

#include "device/masac.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// ------------------------------------------------------------------------------------- critic
// T = r_i + gamma (1 - d_i) (min(Q1', Q2')(s', a') - alpha_i log pi_i(a'_i | s'_i)), a'_j ~ actor_target_j(s'_j) for every j (MASAC.py:214,
// 226-238); mse(Q1, T) + mse(Q2, T); backward -> slab.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void masac_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
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
    g_cf thC = U.theta(2 * ag + 1);
    g_cf tgC = U.target(2 * ag + 1);
    g_f slab = U.slab(2 * ag + 1);
    g_cf ring = U.ring();
    const int am = D.act_max;
    const int heads = NC.heads, ql = NC.n_layers / heads;
    const int OT = R.obs_total, AT = R.act_total, kc0 = NC.L[0].k_pad;
    const float alpha = D.alpha[((size_t)p * n + ag) * 4 + 3];      // the agent's alpha from before this call (its step comes after the actor's)
    const float invB = 1.f / (float)B;

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int nv = c.nv;
    g_ci idx = c.idx;
    g_cf noise_u = c.noise;
    // ---- a'_j, log pi_j = actor_target_j(s'_j) for every agent j (MASAC.py:214): the sample into abuf, the updating agent's log-prob kept
    float lp_next = 0.f;
    for (int j = 0; j < n; ++j) {
        const NetDesc& NJ = D.net[2 * j];
        g_cf tgJ = U.target(2 * j);
        const int Oj = R.obs_dim[j], Aj = R.act_dim[j], cj = R.act_off[j] - R.act_off[0];
        g_cf noise0 = noise_u + (size_t)j * D.batch_max * am;
        gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[j], Oj, 0);
        zero_cols(S.xin, S.xp, rc, Oj, NJ.L[0].k_pad);
        FRL_PHASE(S);
        mlp_fwd_rows(NJ, 0, NJ.n_layers, tgJ, S, ACT_NONE, [&](int r) {
            lds_cf o = S.outb + r * S.op;
            float lp = 0.f;
            for (int c = 0; c < Aj; ++c) {
                const float eps = (r < nv) ? noise0[(size_t)r * am + c] : 0.f;
                S.abuf[r * S.ap + cj + c] = sac_sample(o[c], o[Aj + c], eps, lp);
            }
            if (j == ag) lp_next = lp;
        });
    }
    // ---- the twin target critic on [next_obs_all | a'_all], the minimum per row
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], OT, 0);
    joint_actions_to_xin(S, OT, AT, kc0);
    FRL_PHASE(S);
    const float q = target_q_min(NC, tgC, S);
    if (threadIdx.x < nv) {
        g_cf rec = ring + (size_t)idx[threadIdx.x] * R.stride;
        S.y[threadIdx.x] = td_target_sac(rec[R.rew_off + ag], rec[R.done_off + ag], a.gamma, q, alpha, lp_next);
    }
    FRL_PHASE(S);

    // ---- both online heads on the stored row: forward, MSE delta, backward
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], OT + AT, 0);
    zero_cols(S.xin, S.xp, rc, OT + AT, kc0);
    critic_heads_td(NC, thC, slab, S, a, nv, c.gs, invB, lossp);
    }
    store_loss_part(U, S, lossp);
}

// -------------------------------------------------------------------------------------- actor
// For the ONE agent i = a.agent of every learner (MASAC.py:254-267): a_j = actor_j(s_j) freshly sampled for every j (draw set n + j);
// q = min(Q1, Q2)(s, a) through critic i as the critic Adam has just stepped it; the entropy from a SECOND draw of actor i (set 2 n);
// loss = mean(-q + alpha_i log pi2).  dQ/da_i of both heads by dX-only backwards, the row's minimising head's kept (a tie: half of
// each, as torch.min(a, b)'s backward); the head delta of [mean | log_std] from both routes; actor i's backward -> slab.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void masac_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count, a.agent);
    if (U.none) return;
    const int n = D.n_agents, p = U.p, ag = U.ag;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[2 * ag];
    const NetDesc& NC = D.net[2 * ag + 1];
    const Lds S = carve(D, smem);
    const MasacLds M = carve_masac(D, S, smem);
    const int rc = D.rc, B = a.batch;
    const RowWalk W = U.walk(B);
    g_cf thA = U.theta(2 * ag);
    g_cf thC = U.theta(2 * ag + 1);
    g_f slab = U.slab(2 * ag);
    g_cf ring = U.ring();
    const int am = D.act_max;
    const int ql = NC.n_layers / NC.heads;
    const int OT = R.obs_total, AT = R.act_total, kc0 = NC.L[0].k_pad;
    const int Oa = R.obs_dim[ag], Aa = R.act_dim[ag], acol = R.act_off[ag] - R.act_off[0];
    const float alpha = D.alpha[((size_t)p * n + ag) * 4 + 3];
    const float invB = 1.f / (float)B;
    const int ct0 = (OT + acol) / 16, ct1 = (OT + acol + Aa + 15) / 16;
    const size_t set = (size_t)D.batch_max * am;

    FRL_GLB f32x4* spill = U.spill();
    float alossp = 0.f, entp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, nv = c.nv;
    g_ci idx = c.idx;
    g_cf noise_u = c.noise;
    g_cf eps_own = noise_u + (size_t)(n + ag) * set, eps_ent = noise_u + (size_t)(2 * n) * set;
    // -- a_j = actor_j(s_j) for every agent, the updating one LAST: its hidden rows stay in h1 / h2 until they are parked in act_spill
    //    (the critic passes reuse h1 / h2, as in ac_actor_kernel), its head row goes to M.head, its second draw's log-prob to lp2
    float lp2 = 0.f;
    for (int jj = 0; jj < n; ++jj) {
        const int j = jj == n - 1 ? ag : (jj < ag ? jj : jj + 1);
        const bool own = (j == ag);
        const NetDesc& NJ = D.net[2 * j];
        g_cf thJ = U.theta(2 * j);
        const int Oj = R.obs_dim[j], Aj = R.act_dim[j], cj = R.act_off[j] - R.act_off[0];
        g_cf eps1 = noise_u + (size_t)(n + j) * set;
        gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[j], Oj, 0);
        zero_cols(S.xin, S.xp, rc, Oj, NJ.L[0].k_pad);
        FRL_PHASE(S);
        mlp_fwd_rows(NJ, 0, NJ.n_layers, thJ, S, ACT_NONE, [&](int r) {
            lds_cf o = S.outb + r * S.op;
            float lp = 0.f, l2 = 0.f;
            for (int c = 0; c < Aj; ++c) {
                const float mean = o[c], raw = o[Aj + c];
                S.abuf[r * S.ap + cj + c] = sac_sample(mean, raw, (r < nv) ? eps1[(size_t)r * am + c] : 0.f, lp);
                if (own) {
                    (void)sac_sample(mean, raw, (r < nv) ? eps_ent[(size_t)r * am + c] : 0.f, l2);
                    M.head[r * M.sp + c] = mean;
                    M.head[r * M.sp + Aj + c] = raw;
                }
            }
            if (own) lp2 = l2;
        }, [&]() {
            if (own) park_hidden(S, spill);
        });
    }
    // -- Q1, Q2 on [obs_all | a_all] and dQ_h / da_i of each head; the row's weight of head 0 in S.y once both values are known
    float q0 = 0.f, q1 = 0.f;
    for (int h = 0; h < 2; ++h) {
        gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], OT, 0);
        joint_actions_to_xin(S, OT, AT, kc0);
        FRL_PHASE(S);
        const int npad = NC.L[h * ql + ql - 1].n_pad;
        mlp_fwd_rows(NC, h * ql, ql, thC, S, ACT_NONE, [&](int r) {
            lds_f o = S.outb + r * S.op;
            if (h == 0) q0 = o[0];
            else {
                q1 = o[0];
                S.y[r] = q0 < q1 ? 1.f : (q0 == q1 ? 0.5f : 0.f);
            }
            o[0] = (r < nv) ? -invB : 0.f;
            for (int c = 1; c < npad; ++c) o[c] = 0.f;
        });
        mlp_bwd(NC, h * ql, ql, thC, nullptr, S, GS_ADD, true, ct0, ct1);
        for (int e = threadIdx.x; e < rc * Aa; e += kWG) {
            const int r = e / Aa, c = e - r * Aa;
            const float g = S.xin[r * S.xp + OT + acol + c];
            if (h == 0) S.dabuf[r * S.ap + c] = g;
            else {
                const float w0 = S.y[r];
                S.dabuf[r * S.ap + c] = w0 * S.dabuf[r * S.ap + c] + (1.f - w0) * g;
            }
        }
        FRL_PHASE(S);
    }
    if (threadIdx.x < nv) {
        alossp += -fminf(q0, q1) + alpha * lp2;       // (-q_pi - alpha entropy), MASAC.py:266
        entp += -lp2;
    }
    // -- the actor's activations back (same thread, same addresses as the spill), its input back in xin, the head delta of both routes
    restore_hidden(S, spill);
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[ag], Oa, 0);
    zero_cols(S.xin, S.xp, rc, Oa, NA.L[0].k_pad);
    const int napad = NA.L[NA.n_layers - 1].n_pad;
    for (int e = threadIdx.x; e < rc * napad; e += kWG) {
        const int r = e / napad, c = e - r * napad;
        float d = 0.f;
        if (r < nv && c < 2 * Aa) {
            const int cc = c < Aa ? c : c - Aa;
            const float mean = M.head[r * M.sp + cc], raw = M.head[r * M.sp + Aa + cc];
            const float e1 = eps_own[(size_t)r * am + cc], e2 = eps_ent[(size_t)r * am + cc];
            const float a1 = S.abuf[r * S.ap + acol + cc], dq = S.dabuf[r * S.ap + cc];
            const float t2 = tanhf(mean + expf(clamp_log_std(raw)) * e2);
            d = c < Aa ? sac2_mean_delta(dq, a1, t2, alpha, invB) : sac2_log_std_delta(dq, a1, t2, raw, e1, e2, alpha, invB);
        }
        S.outb[r * S.op + c] = d;
    }
    FRL_PHASE(S);
    mlp_bwd(NA, 0, NA.n_layers, thA, slab, S, gs, false, 0, 0);
    }
    const float la = block_sum(alossp, S.red);
    const float le = block_sum(entp, S.red);
    store_loss_parts(U, la, le);
}

// ------------------------------------------------------------------------------------ forward
// frl_act on an actor (net 2i) of an ALGO_MASAC engine: FRL_ACT_TANHHEAD = tanh(mean) (evaluate_action, MASAC.py:194), FRL_ACT_SAC_SAMPLE =
// tanh(mean + exp(clamp(log_std)) eps) (select_action, :182); act_dim columns out.  grid = (row chunks, learners).
__global__ __launch_bounds__(256) void masac_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc;
    const NetDesc& N = D.net[a.net];
    const Lds S = carve(D, smem);
    const int rc = D.rc, nv = min(rc, a.n_rows - r0);
    const int K = a.in_dim, kp = N.L[0].k_pad, A = N.L[N.n_layers - 1].n / 2;
    g_cf theta = as_global((a.use_target ? D.target : D.theta) + (size_t)p * D.learner_stride + D.net_off[a.net]);
    g_cf in = as_global(a.in + ((size_t)p * a.n_rows + r0) * K);
    load_rows(S.xin, S.xp, rc, nv, in, 0, K, 0, K, kp);
    __syncthreads();
    mlp_fwd(N, 0, N.n_layers, theta, S, ACT_NONE);
    for (int e = threadIdx.x; e < nv * A; e += kWG) {
        const int r = e / A, c = e - r * A;
        const size_t o = ((size_t)p * a.n_rows + r0 + r) * A + c;
        const float mean = S.outb[r * S.op + c];
        float v;
        if (a.mode == ACTM_SAC_SAMPLE) {
            float lp = 0.f;
            v = sac_sample(mean, S.outb[r * S.op + A + c], a.eps[o], lp);
        } else {
            v = tanhf(mean);
        }
        a.out[o] = v;
    }
}

}  // namespace frl
