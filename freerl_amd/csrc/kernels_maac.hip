// MAAC (MAAC_file/MAAC_discrete.py:208-280 with Attention.py: Iqbal & Sha's Actor-Attention-Critic, discrete actors, alpha a constant): the
// kernels of an ALGO_MAAC engine.  Per agent i, in agent order, frl_learn launches
//     maac_critic_kernel -> maac_reduce_kernel -> maac_step_kernel -> maac_actor_kernel -> reduce + clip + Adam of actor i (kernels_update.hip)
// and behind all agents the soft stage (soft_update_kernel for the 2 n nets, maac_soft_kernel for the n target attention blocks).  The
// order is the algorithm: ONE attention block is shared by every online critic, so critic i + 1 must read it as critic i's Adam left it,
// and actor i reads critic i and the actors j < i as just stepped.  Stream order carries all of that.
// The gradient kernels are row-chunk kernels on update_common.hpp's skeleton: units = the learners, for the ONE agent LearnArgs::agent; a
// workgroup walks its `cps` chunks of 16 rows through RowWalk and leaves one gradient slab (the own net's region and attention slot i).
// Draw sets of D.noise (Exp(1) draws), per updating agent: j = target actor j, n + j = online actor j's draw 1, 2 n = the second draw of actor i.
#include <hip/hip_runtime.h>

#include "device/maac.hpp"
#include "kernels.h"

namespace frl {

// one-hot of a row's draw into the joint action block abuf (cj: the agent's first column there)
__device__ __forceinline__ void maac_onehot(const Lds& S, int r, int cj, int A, int k) {
    for (int c = 0; c < A; ++c) S.abuf[r * S.ap + cj + c] = (c == k) ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------- critic
// T = r_i + gamma (1 - d_i)(all_q'[a'_i] - alpha_i log pi'_i(a'_i)), a'_j ~ actor_target_j(o'_j) for every j, all_q' the TARGET critic i on
// (o', a'); mse(all_q[stored a_i], T) on the stored row; the closed-form backward -> slab.
__global__ __launch_bounds__(256, 1) void maac_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count, a.agent);
    if (U.none) return;
    const int n = D.n_agents, p = U.p, ag = U.ag;
    const RecordDesc& R = D.rec;
    const Lds S = carve(D, smem);
    const MaacLds A = carve_maac(S, n);
    const int B = a.batch, am = D.act_max;
    const RowWalk W = U.walk(B, true);
    g_cf th_online = as_global(D.theta + U.lbase());
    const MaacCritic CT{D.net[2 * ag + 1], D.maac_att, U.target(2 * ag + 1), as_global(D.target + U.lbase() + maac_att_offset(D, ag)), th_online, ag};
    const MaacCritic CO{D.net[2 * ag + 1], D.maac_att, U.theta(2 * ag + 1), as_global(D.theta + U.lbase() + maac_att_offset(D, 0)), th_online, ag};
    g_f G = U.slab(2 * ag + 1);
    g_f GA = as_global(D.slab + maac_att_slab_offset(D, p, U.sl, ag));
    g_cf ring = U.ring();
    const int Ai = R.act_dim[ag], npad = CO.NC.L[MAAC_FC2].n_pad;
    const float alpha = D.alpha[((size_t)p * n + ag) * 4 + 3];
    const float invB = 1.f / (float)B;
    const size_t set = noise_set_floats(D);

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int nv = c.nv;
    g_ci idx = c.idx;
    // ---- a'_j ~ actor_target_j(o'_j) for every agent j (draw set j): one-hot into abuf, the updating agent's index and log-prob kept
    int a_next = 0;
    float lp_next = 0.f;
    for (int j = 0; j < n; ++j) {
        const NetDesc& NJ = D.net[2 * j];
        const int Oj = R.obs_dim[j], Aj = R.act_dim[j], cj = R.act_off[j] - R.act_off[0];
        g_cf q = c.noise + (size_t)j * set;
        gather_cols(S.xin, S.xp, S.rc, nv, idx, ring, R.stride, R.nobs_off[j], Oj, 0);
        zero_cols(S.xin, S.xp, S.rc, Oj, NJ.L[0].k_pad);
        FRL_PHASE(S);
        mlp_fwd_rows(NJ, 0, NJ.n_layers, U.target(2 * j), S, ACT_NONE, [&](int r) {
            lds_cf z = S.outb + r * S.op;
            int k = 0;
            if (r < nv) {
                const MaacSoftmax m = maac_softmax(z, Aj);
                k = maac_draw(m, z, Aj, q + (size_t)r * am);
                if (j == ag) { a_next = k; lp_next = maac_logp(m, z[k]); }
            }
            maac_onehot(S, r, cj, Aj, r < nv ? k : -1);
        }, NoRowConsumer{}, std::true_type{});
    }
    // ---- the target critic on (o', a'), the others streamed; the TD target per row
    const MaacRows next{ring, idx, R.stride, nv, 1, S.abuf};
    maac_fwd(D, CT, S, A, next);
    if (threadIdx.x < nv) {
        g_cf rec = ring + (size_t)idx[threadIdx.x] * R.stride;
        S.y[threadIdx.x] = td_target_sac(rec[R.rew_off + ag], rec[R.done_off + ag], a.gamma, S.outb[threadIdx.x * S.op + a_next], alpha, lp_next);
    }
    FRL_PHASE(S);
    // ---- the online critic on the stored row; the delta in the stored action's column only
    const MaacRows cur{ring, idx, R.stride, nv, 0, nullptr};
    maac_fwd(D, CO, S, A, cur);
    if (threadIdx.x < S.rc) {
        const int r = threadIdx.x;
        lds_f o = S.outb + r * S.op;
        int pick = -1;
        float d = 0.f;
        if (r < nv) {
            g_cf act = ring + (size_t)idx[r] * R.stride + R.act_off[ag];
            pick = 0;
            for (int k = 1; k < Ai; ++k)
                if (act[k] > act[pick]) pick = k;
            const float dl = o[pick] - S.y[r];
            lossp += dl * dl;
            d = dl * (2.f * invB);
        }
        for (int k = 0; k < npad; ++k) o[k] = (k == pick) ? d : 0.f;
    }
    FRL_PHASE(S);
    maac_bwd(D, CO, G, GA, S, A, cur, c.gs);
    }
    store_loss_part(U, S, lossp);
}

// -------------------------------------------------------------------------------------- actor
// For agent i = a.agent of every learner: a_j ~ actor_j(o_j) for the others (draw set n + j; j < i as just stepped); all_q of critic i on
// (o, a) as its Adam has just left it — forward only; actor i's own forward LAST, so that its activations are still in LDS for its backward:
// draw 1 (set n + i) picks q_pi, draw 2 (set 2 n) gives log_pi; v = sum_k all_q[k] p_k; loss = mean(log_pi (v - q_pi + alpha log_pi));
// d z_k = [(v - q_pi + 2 alpha lp)(1[k = a2] - p_k) + lp p_k (all_q[k] - v)] / B; actor i's backward -> slab.
__global__ __launch_bounds__(256, 1) void maac_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count, a.agent);
    if (U.none) return;
    const int n = D.n_agents, p = U.p, ag = U.ag;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[2 * ag];
    const Lds S = carve(D, smem);
    const MaacLds A = carve_maac(S, n);
    const int B = a.batch, am = D.act_max;
    const RowWalk W = U.walk(B);
    g_cf th_online = as_global(D.theta + U.lbase());
    const MaacCritic CO{D.net[2 * ag + 1], D.maac_att, U.theta(2 * ag + 1), as_global(D.theta + U.lbase() + maac_att_offset(D, 0)), th_online, ag};
    g_cf thA = U.theta(2 * ag);
    g_f slab = U.slab(2 * ag);
    g_cf ring = U.ring();
    const int Oi = R.obs_dim[ag], Ai = R.act_dim[ag], napad = NA.L[NA.n_layers - 1].n_pad;
    const float alpha = D.alpha[((size_t)p * n + ag) * 4 + 3];
    const float invB = 1.f / (float)B;
    const size_t set = noise_set_floats(D);

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int nv = c.nv;
    g_ci idx = c.idx;
    for (int j = 0; j < n; ++j) {
        if (j == ag) continue;      // (critic i does not read a_i: all_q has a column per own action)
        const NetDesc& NJ = D.net[2 * j];
        const int Oj = R.obs_dim[j], Aj = R.act_dim[j], cj = R.act_off[j] - R.act_off[0];
        g_cf q = c.noise + (size_t)(n + j) * set;
        gather_cols(S.xin, S.xp, S.rc, nv, idx, ring, R.stride, R.obs_off[j], Oj, 0);
        zero_cols(S.xin, S.xp, S.rc, Oj, NJ.L[0].k_pad);
        FRL_PHASE(S);
        mlp_fwd_rows(NJ, 0, NJ.n_layers, U.theta(2 * j), S, ACT_NONE, [&](int r) {
            lds_cf z = S.outb + r * S.op;
            int k = -1;
            if (r < nv) k = maac_draw(maac_softmax(z, Aj), z, Aj, q + (size_t)r * am);
            maac_onehot(S, r, cj, Aj, k);
        }, NoRowConsumer{}, std::true_type{});
    }
    const MaacRows cur{ring, idx, R.stride, nv, 0, S.abuf};
    maac_fwd(D, CO, S, A, cur);
    for (int e = threadIdx.x; e < S.rc * Ai; e += kWG) {      // all_q parked in dabuf: the actor's head reuses outb
        const int r = e / Ai, k = e - r * Ai;
        S.dabuf[r * S.ap + k] = S.outb[r * S.op + k];
    }
    gather_cols(S.xin, S.xp, S.rc, nv, idx, ring, R.stride, R.obs_off[ag], Oi, 0);
    zero_cols(S.xin, S.xp, S.rc, Oi, NA.L[0].k_pad);
    FRL_PHASE(S);
    g_cf q1 = c.noise + (size_t)(n + ag) * set, q2 = c.noise + (size_t)(2 * n) * set;
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_NONE, [&](int r) {
        lds_f z = S.outb + r * S.op;
        if (r < nv) {
            lds_cf aq = S.dabuf + r * S.ap;
            const MaacSoftmax m = maac_softmax(z, Ai);
            const int a1 = maac_draw(m, z, Ai, q1 + (size_t)r * am), a2 = maac_draw(m, z, Ai, q2 + (size_t)r * am);
            const float lp = maac_logp(m, z[a2]), qpi = aq[a1];
            float v = 0.f;
            for (int k = 0; k < Ai; ++k) v += aq[k] * maac_prob(m, z[k]);
            const float w = v - qpi + 2.f * alpha * lp;
            lossp += lp * (v - qpi + alpha * lp);
            for (int k = 0; k < Ai; ++k) {
                const float pk = maac_prob(m, z[k]);
                z[k] = (w * ((k == a2 ? 1.f : 0.f) - pk) + lp * pk * (aq[k] - v)) * invB;
            }
            for (int k = Ai; k < napad; ++k) z[k] = 0.f;
        } else {
            for (int k = 0; k < napad; ++k) z[k] = 0.f;
        }
    }, NoRowConsumer{}, std::true_type{});
    mlp_bwd(NA, 0, NA.n_layers, thA, slab, S, c.gs, false, 0, 0, std::true_type{});
    }
    store_loss_part(U, S, lossp);
}

// ------------------------------------------------------------------- reduce + clip + Adam of ONE critic
// The 12 trained tensors of critic i = a.agent1 - 1 sit in two storage regions (its own net, attention slot i of the slabs); both kernels
// walk them as the one float4 index space of maac_trained_at, a.G workgroups per learner, grid-strided.
//   maac_reduce_kernel: g = sum over the slabs in slice order (deterministic) -> D.grad; a workgroup's sum of squares -> gsq; workgroup 0
//                       advances the critic's Adam step count.
//   maac_step_kernel  : ONE global norm from gsq -> clip_grad_norm_'s coefficient -> torch-order Adam.  The attention tensors take agent
//                       i's moments (slot i of m / v) and write the SHARED online block (slot 0 of theta).  The frozen eight are in no range.
__global__ __launch_bounds__(256) void maac_reduce_kernel(const EngineDesc* __restrict__ Dp, AdamArgs a) {
    __shared__ float red_s[8];
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, wg = blockIdx.x % a.G, p = a.p0 + blockIdx.x / a.G, ag = a.agent1 - 1, net = 2 * ag + 1;
    const NetDesc& NC = D.net[net];
    const NetDesc& NA = D.maac_att;
    const size_t lb = (size_t)p * D.learner_stride, ls4 = (size_t)D.learner_stride / 4;
    const FRL_GLB f32x4* slabC = (const FRL_GLB f32x4*)(D.slab + slab_offset(D, p, 0, net));
    const FRL_GLB f32x4* slabA = (const FRL_GLB f32x4*)(D.slab + maac_att_slab_offset(D, p, 0, ag));
    FRL_GLB f32x4* gC = (FRL_GLB f32x4*)(D.grad + lb + D.net_off[net]);
    FRL_GLB f32x4* gA = (FRL_GLB f32x4*)(D.grad + lb + maac_att_offset(D, ag));
    const int total = maac_trained4(NC, NA);
    float ss = 0.f;
    for (int v = wg * kWG + threadIdx.x; v < total; v += a.G * kWG) {
        int off4;
        bool att;
        maac_trained_at(NC, NA, v, off4, att);
        const FRL_GLB f32x4* src = (att ? slabA : slabC) + off4;
        f32x4 s = src[0];
        for (int k = 1; k < a.ns; ++k) s += src[(size_t)k * ls4];
        (att ? gA : gC)[off4] = s;
        ss += s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
    }
    const float tot = block_sum(ss, (lds_f)red_s);
    if (threadIdx.x == 0) {
        D.gsq[((size_t)p * n + ag) * D.Gmax + wg] = tot;
        if (wg == 0) D.steps[(size_t)p * (kMaxNets + 1) + net] += 1;
    }
}

__global__ __launch_bounds__(256) void maac_step_kernel(const EngineDesc* __restrict__ Dp, AdamArgs a) {
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, wg = blockIdx.x % a.G, p = a.p0 + blockIdx.x / a.G, ag = a.agent1 - 1, net = 2 * ag + 1;
    const NetDesc& NC = D.net[net];
    const NetDesc& NA = D.maac_att;
    float ss = 0.f;
    for (int k = 0; k < a.G; ++k) ss += D.gsq[((size_t)p * n + ag) * D.Gmax + k];      // same order in every workgroup
    const float total = sqrtf(ss);
    const int t = D.steps[(size_t)p * (kMaxNets + 1) + net];                            // advanced by maac_reduce_kernel
    const AdamCoef c = adam_coef(total, a.clip, t, a.lr, a.beta1, a.beta2, a.eps, 0.f, 0.f);
    const size_t lb = (size_t)p * D.learner_stride, offC = lb + D.net_off[net], offA = lb + maac_att_offset(D, ag), offT = lb + maac_att_offset(D, 0);
    const int n4 = maac_trained4(NC, NA);
    for (int v = wg * kWG + threadIdx.x; v < n4; v += a.G * kWG) {
        int off4;
        bool att;
        maac_trained_at(NC, NA, v, off4, att);
        const size_t og = (att ? offA : offC) + 4 * (size_t)off4, ot = (att ? offT : offC) + 4 * (size_t)off4;
        g_f th = as_global(D.theta + ot), m = as_global(D.m + og), vv = as_global(D.v + og);
        f32x4 mi = ld4((g_cf)m), vi = ld4((g_cf)vv);
        const f32x4 x = adam_exact4(ld4((g_cf)th), ld4(as_global(D.grad + og)) * c.coef, mi, vi, c.w1, c.w2, a.beta2, c.bc2s, a.eps, c.step);
        st4(m, mi);
        st4(vv, vi);
        st4(th, x);
    }
    if (wg == 0 && threadIdx.x == 0) {
        const float* pt = D.part + part_offset(D, p, ag, 0);
        float l0 = 0.f;
        for (int k = 0; k < a.ns; ++k) l0 += pt[kPartFloats * k];
        float* st = D.stats + ((size_t)p * n + ag) * ST_COUNT;
        st[ST_CRITIC_LOSS] = l0 / (float)a.batch;
        st[ST_CRITIC_GNORM] = total;
        st[ST_ALPHA] = D.alpha[((size_t)p * n + ag) * 4 + 3];
    }
}

// the n target attention blocks (slot i of target) towards the ONE online block (slot 0 of theta); grid = (learners x agents, pieces)
__global__ __launch_bounds__(256) void maac_soft_kernel(const EngineDesc* __restrict__ Dp, float tau, int p0) {
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, p = p0 + blockIdx.x / n, ag = blockIdx.x % n;
    const size_t lb = (size_t)p * D.learner_stride;
    g_f tg = as_global(D.target + lb + maac_att_offset(D, ag));
    g_cf th = as_global(D.theta + lb + maac_att_offset(D, 0));
    const float tk = 1.f - tau;
    for (int i = blockIdx.y * kWG + threadIdx.x; i < D.maac_att.size; i += gridDim.y * kWG) tg[i] = tg[i] * tk + th[i] * tau;
}

// a device-drawn call's Exp(1) draws for every (learner, updating agent, set): -log(u), u uniform on (0, 1] from the call's Philox counter
// (behind draw_kernel, which draws the rows).  grid = learners x agents
__global__ __launch_bounds__(256) void maac_noise_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a) {
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, p = a.p0 + blockIdx.x / n, ag = blockIdx.x % n, am = D.act_max;
    const unsigned long long key = D.seed + 0x9E3779B97F4A7C15ull * (p + 1);
    for (int s = 0; s < D.noise_sets; ++s) {
        g_f q = as_global(D.noise + noise_offset(D, p, ag, s, 0));
        for (int e = threadIdx.x; e < a.batch * am; e += kWG)
            q[e] = fmaxf(-logf(u01(philox4x32_10(a.rng_counter, 0x6000u + (unsigned)ag + 0x100u * (unsigned)s, (unsigned)e, key).x)), 1e-30f);
    }
}

// ------------------------------------------------------------------------------------ forward
// frl_act on an actor (net 2i): FRL_ACT_CAT_SAMPLE = the draw's index (select_action; a.eps: Exp(1) draws [P][n_rows][A]), FRL_ACT_ARGMAX the
// most probable action, FRL_ACT_RAW the logits.  grid = (row chunks, learners).
__global__ __launch_bounds__(256) void maac_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc;
    const NetDesc& N = D.net[a.net];
    const Lds S = carve(D, smem);
    const int nv = min(S.rc, a.n_rows - r0), K = a.in_dim, A = N.L[N.n_layers - 1].n;
    g_cf theta = as_global((a.use_target ? D.target : D.theta) + (size_t)p * D.learner_stride + D.net_off[a.net]);
    load_rows(S.xin, S.xp, S.rc, nv, as_global(a.in + ((size_t)p * a.n_rows + r0) * K), 0, K, 0, K, N.L[0].k_pad);
    __syncthreads();
    mlp_fwd_rows(N, 0, N.n_layers, theta, S, ACT_NONE, [&](int r) {
        if (r >= nv) return;
        lds_cf z = S.outb + r * S.op;
        const size_t row = (size_t)p * a.n_rows + r0 + r;
        if (a.mode == ACTM_RAW) {
            for (int k = 0; k < A; ++k) a.out[row * A + k] = z[k];
            return;
        }
        const MaacSoftmax m = maac_softmax(z, A);
        int k = 0;
        if (a.mode == ACTM_CAT_SAMPLE) k = maac_draw(m, z, A, as_global(a.eps + row * A));
        else
            for (int c = 1; c < A; ++c)
                if (z[c] > z[k]) k = c;
        a.out[row] = (float)k;
        if (a.out_logp) a.out_logp[row] = maac_logp(m, z[k]);
    }, NoRowConsumer{}, std::true_type{});
}

// frl_act (FRL_ACT_RAW) on a critic (net 2i+1): all_q of rows [obs_0 .. obs_{n-1} | act_0 .. act_{n-1}] (one-hot actions), A_i columns out:
// agents[i].critic(obs_list, act_list), or critic_target's with use_target.  grid = (row chunks, learners).
__global__ __launch_bounds__(256) void maac_q_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc, ag = a.net / 2;
    const Lds S = carve(D, smem);
    const MaacLds A = carve_maac(S, D.n_agents);
    const int nv = min(S.rc, a.n_rows - r0), K = a.in_dim, Ai = D.rec.act_dim[ag];
    const size_t lb = (size_t)p * D.learner_stride;
    g_cf base = as_global((a.use_target ? D.target : D.theta) + lb);
    const MaacCritic C{D.net[a.net], D.maac_att, base + D.net_off[a.net], base + maac_att_offset(D, a.use_target ? ag : 0), as_global(D.theta + lb), ag};
    const MaacRows rows{as_global(a.in + ((size_t)p * a.n_rows + r0) * K), nullptr, K, nv, 0, nullptr};
    maac_fwd(D, C, S, A, rows);
    for (int e = threadIdx.x; e < nv * Ai; e += kWG) {
        const int r = e / Ai, k = e - r * Ai;
        a.out[((size_t)p * a.n_rows + r0 + r) * Ai + k] = S.outb[r * S.op + k];
    }
}

}  // namespace frl
