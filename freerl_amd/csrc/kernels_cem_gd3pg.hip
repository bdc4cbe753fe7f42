// CEM_GD3PG (CEM_GD3PG_file/CEM_GD3PG.py:94-231: guided dual-actor DDPG, the gradient half of CEM-GD3PG) on the row-chunk skeleton: the
// critic-then-actor shape of kernels_envelope_ddpg.hip with two online actors, a frozen domain actor and one critic per learner.
// Launch chain (frl_api_cem_gd3pg.inc):
//     [cem_draw_kernel] -> cem_critic_kernel -> cem_step_kernel (critic) -> cem_actor_kernel (both actors) -> cem_step_kernel (actors)
// Net 0 is actor_1, net 1 actor_2, net 3 actor_domain (obs -> H tanh -> H tanh -> A tanh), net 2 the critic on [obs | act] (H LeakyReLU ->
// H LeakyReLU -> 1).  The batch's B = 2 half rows are absolute rows of the learner's two rings in idx (half of `buffer`, then half of
// `buffer_domain`), so no kernel here knows about rings.
// The guided actor's penalty lambda delta sqrt(sum c^2 / B), c = actor_g(s) - actor_domain(s), needs a sum over the WHOLE batch before
// that actor's backward.  Nothing it reads changes in the critic step, so cem_critic_kernel forms it: every workgroup leaves its rows'
// sum c^2 in its part slot and the domain actor's rows in HBM; cem_actor_kernel adds the slots up (cem_c2_sum) and reads the rows back.
// cem_step_kernel is reduce + clip + Adam + soft update for three trained nets per learner: the shared launches of kernels_update.hip
// address a unit's nets as (actor 2 ag, critic 2 ag + 1) and publish two statistics, so this one sums the slabs itself and then runs
// the same device function (adam_net, device/net.hpp) that PPO's update steps with.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/net.hpp"
#include "device/act_common.hpp"
#include "device/cem.hpp"
#include "device/update_common.hpp"

namespace frl {

using Leaky = std::true_type;      // the critic's hidden activation: mlp_fwd_rows / mlp_bwd's trailing argument

// --------------------------------------------------------------------------------------- draw
// sample() (:160-176): np.random.choice(total, half, replace=False) twice, total = len(buffer_domain) for BOTH draws; the first half
// indexes ring 0, the second ring 1 (absolute rows ring_cap + r).  One workgroup per learner; 2 round_up(half, 4) ints of LDS
__global__ __launch_bounds__(256) void cem_draw_kernel(const EngineDesc* __restrict__ Dp, CemArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = a.p0 + blockIdx.x;
    g_i idx = (g_i)(D.idx + idx_offset(D, p, 0, 0));
    const unsigned long long key = D.seed + 0x9E3779B97F4A7C15ull * (p + 1);
    FRL_LDS int* lb = (FRL_LDS int*)smem;
    draw_indices(idx, lb, a.half, a.size1, a.rng_counter, 0u, key);
    draw_indices(nullptr, lb, a.half, a.size1, a.rng_counter, 1u, key);
    for (int i = threadIdx.x; i < a.half; i += kWG) idx[a.half + i] = a.ring_cap + lb[i];
}

// ------------------------------------------------------------------------------------- critic
// T = r + gamma (1 - done) min(critic_target(s', actor_1_target(s')), critic_target(s', actor_2_target(s'))) (:185-189); loss = mean (critic(s, a)
// - T)^2 (:191-193).  Ahead of the critic's own pass: actor_g(s) and actor_domain(s) of the learner's guided actor g, for sum c^2.
// A target action goes straight into the critic's input row (the actor's first layer has read xin by then); Q1' waits in y, then T.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void cem_critic_kernel(const EngineDesc* __restrict__ Dp, CemArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[CEM_ACTOR_1];            // (the three actors have one shape)
    const NetDesc& NC = D.net[CEM_CRITIC];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.rows;
    const RowWalk W = U.walk(B);
    g_cf tgC = U.target(CEM_CRITIC);
    g_cf thC = U.theta(CEM_CRITIC);
    g_f slab = U.slab(CEM_CRITIC);
    g_cf ring = U.ring();
    const int guided = cem_guided(D, U.p);
    const int O = R.obs_dim[0], A = R.act_dim[0], am = D.act_max;
    const int ka0 = NA.L[0].k_pad, kc0 = NC.L[0].k_pad, npad = NC.L[NC.n_layers - 1].n_pad;

    float lossp = 0.f, c2p = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, nv = c.nv;
    g_ci idx = c.idx;
    // ---- both target actors on s', each followed by the target critic on [s' | a']
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], O, 0);
    for (int t = 0; t < kCemActors; ++t) {
        zero_cols(S.xin, S.xp, rc, O, t == 0 ? kc0 : ka0);      // (the second round: a_1' sits where the actor's first layer reads zeros)
        FRL_PHASE(S);
        mlp_fwd_rows(NA, 0, NA.n_layers, U.target(t), S, ACT_TANH, [&](int r) {
            for (int k = 0; k < A; ++k) S.xin[r * S.xp + O + k] = S.outb[r * S.op + k];
        });
        mlp_fwd_rows(NC, 0, NC.n_layers, tgC, S, ACT_NONE, [&](int r) {
            const float q = S.outb[r * S.op];
            if (t == 0) { S.y[r] = q; return; }
            float T = 0.f;
            if (r < nv) {
                g_cf rec = ring + (size_t)idx[r] * R.stride;
                T = rec[R.rew_off] + a.gamma * fminf(S.y[r], q) * (1.f - rec[R.done_off]);
            }
            S.y[r] = T;
        }, NoRowConsumer{}, Leaky{});
    }
    // ---- the guided actor and the domain actor on s: the rows' sum c^2, the domain actor's rows parked for cem_actor_kernel
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);
    zero_cols(S.xin, S.xp, rc, O, ka0);
    FRL_PHASE(S);
    mlp_fwd_rows(NA, 0, NA.n_layers, U.theta(guided), S, ACT_TANH, [&](int r) {
        for (int k = 0; k < A; ++k) S.abuf[r * S.ap + k] = S.outb[r * S.op + k];
    });
    g_f dom = cem_domain_rows(U, c.r0);
    mlp_fwd_rows(NA, 0, NA.n_layers, U.theta(CEM_DOMAIN), S, ACT_TANH, [&](int r) {
        if (r >= nv) return;
        for (int k = 0; k < A; ++k) {
            const float ad = S.outb[r * S.op + k], d = S.abuf[r * S.ap + k] - ad;
            dom[(size_t)r * am + k] = ad;
            c2p += d * d;
        }
    });
    // ---- critic on [s | a] (adjacent in a record), the TD delta, backward
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O + A, 0);
    zero_cols(S.xin, S.xp, rc, O + A, kc0);
    FRL_PHASE(S);
    mlp_fwd_rows(NC, 0, NC.n_layers, thC, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        float d = 0.f;
        if (r < nv) {
            const float e = o[0] - S.y[r];
            lossp += e * e;
            d = 2.f * e / (float)B;
        }
        o[0] = d;
        for (int k = 1; k < npad; ++k) o[k] = 0.f;
    }, NoRowConsumer{}, Leaky{});
    mlp_bwd(NC, 0, NC.n_layers, thC, slab, S, gs, false, 0, 0, Leaky{});
    }
    const float ls = block_sum(lossp, S.red), c2 = block_sum(c2p, S.red);
    if (threadIdx.x == 0) {
        float* pt = U.part();
        pt[CEM_PART_CRITIC] = ls;
        pt[CEM_PART_C2] = c2;
    }
}

// -------------------------------------------------------------------------------------- actor
// Unit (learner, actor j): a = actor_j(s); loss = -mean Q(s, a) through the critic just stepped (:198-199), plus lambda delta KL when j is
// the guided one (:205-207 / :213-215).  Head delta of row r, column k: (-(1/B) dQ/da + [guided] lambda delta c / (B KL)) tanh'; the
// critic's constant head delta -1/B, a dX-only backward to the action's column tiles, then the actor's backward — ac_actor_kernel's shape.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void cem_actor_kernel(const EngineDesc* __restrict__ Dp, CemArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    int actor;
    const RowUnit U = cem_actor_unit(D, ns, a.p0, a.p_count, actor);
    if (U.none) return;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[actor];
    const NetDesc& NC = D.net[CEM_CRITIC];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.rows;
    const RowWalk W = U.walk(B);
    g_cf thA = U.theta(actor);
    g_cf thC = U.theta(CEM_CRITIC);
    g_f slab = U.slab(actor);
    g_cf ring = U.ring();
    const int O = R.obs_dim[0], A = R.act_dim[0], am = D.act_max;
    const int ka0 = NA.L[0].k_pad, kc0 = NC.L[0].k_pad;
    const int ncpad = NC.L[NC.n_layers - 1].n_pad, napad = NA.L[NA.n_layers - 1].n_pad;
    const int ct0 = O / 16, ct1 = (O + A + 15) / 16;            // the action's column tiles of the critic's input
    const float dq = -1.f / (float)B;
    // the penalty's gradient per unit of c: lambda delta / (B KL); 0 for the unguided actor and where sum c^2 == 0
    float pen = 0.f;
    if (actor == cem_guided(D, U.p)) {
        const float kl = cem_kl(cem_c2_sum(D, U.p, ns), B);
        if (kl > 0.f) pen = a.lambda * cem_delta(D, U.p) / ((float)B * kl);
    }
    FRL_GLB f32x4* spill = cem_spill(U, actor);

    float alossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, nv = c.nv;
    g_ci idx = c.idx;
    // ---- a = actor(s): kept in abuf for tanh' and c, and written into the critic's input row
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);
    zero_cols(S.xin, S.xp, rc, O, kc0);
    FRL_PHASE(S);
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_TANH, [&](int r) {
        for (int k = 0; k < A; ++k) {
            const float av = S.outb[r * S.op + k];
            S.abuf[r * S.ap + k] = av;
            S.xin[r * S.xp + O + k] = av;
        }
    }, [&]() { park_hidden(S, spill); });
    // ---- the stepped critic on [s | a]: Q into the loss sum, the constant head delta, dX into the action column tiles
    mlp_fwd_rows(NC, 0, NC.n_layers, thC, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        const bool live = r < nv;
        if (live) alossp -= o[0];
        o[0] = live ? dq : 0.f;
        for (int k = 1; k < ncpad; ++k) o[k] = 0.f;
    }, NoRowConsumer{}, Leaky{});
    mlp_bwd(NC, 0, NC.n_layers, thC, nullptr, S, GS_ADD, true, ct0, ct1, Leaky{});
    for (int e = threadIdx.x; e < rc * A; e += kWG) {
        const int r = e / A, k = e - r * A;
        S.dabuf[r * S.ap + k] = S.xin[r * S.xp + O + k];
    }
    FRL_PHASE(S);
    // ---- the actor's activations back from HBM (same thread, same addresses as the spill), its input back in xin
    restore_hidden(S, spill);
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);      // (the critic's dX landed on xin)
    zero_cols(S.xin, S.xp, rc, O, ka0);
    // the head delta in the same phase: it reads dabuf / abuf and writes outb, none of which the reload above touches
    g_cf dom = cem_domain_rows(U, c.r0);
    for (int e = threadIdx.x; e < rc * napad; e += kWG) {
        const int r = e / napad, k = e - r * napad;
        float d = 0.f;
        if (r < nv && k < A) {
            const float av = S.abuf[r * S.ap + k];
            float g = S.dabuf[r * S.ap + k];
            if (pen != 0.f) g += pen * (av - dom[(size_t)r * am + k]);
            d = tanh_delta(g, av);
        }
        S.outb[r * S.op + k] = d;
    }
    FRL_PHASE(S);
    mlp_bwd(NA, 0, NA.n_layers, thA, slab, S, gs, false, 0, 0);
    }
    const float la = block_sum(alossp, S.red);
    if (threadIdx.x == 0) U.part()[CEM_PART_ACTOR + actor] = la;
}

// ------------------------------------------------------------------------------- reduce + step
// One workgroup per trained net of the stage: the slices' slabs summed in slice order into the learner's grad block, then
// clip_grad_norm_(0.5) + torch-order Adam + the soft update of the net's target (adam_net), the step count, and the statistics.
// stage 0: the critic of learners p0 ..; stage 1: units (learner, actor)
__global__ __launch_bounds__(256) void cem_step_kernel(const EngineDesc* __restrict__ Dp, CemArgs a, int ns) {
    __shared__ float red_s[8];
    const EngineDesc& D = *Dp;
    const int u = blockIdx.x;
    const int p = a.p0 + (a.stage == 0 ? u : u / kCemActors), net = a.stage == 0 ? (int)CEM_CRITIC : u % kCemActors;
    const NetDesc& N = D.net[net];
    const size_t off = (size_t)p * D.learner_stride + D.net_off[net];
    const int n4 = N.size / 4;                                          // (a net's size is a multiple of 32 floats)
    FRL_GLB f32x4* g = (FRL_GLB f32x4*)(D.grad + off);
    const FRL_GLB f32x4* slab = (const FRL_GLB f32x4*)(D.slab + slab_offset(D, p, 0, net));      // slice 0; slice k lies k learner strides further
    const size_t ls4 = (size_t)D.learner_stride / 4;
    for (int i = threadIdx.x; i < n4; i += kWG) {
        f32x4 s = slab[i];
        for (int k = 1; k < ns; ++k) s += slab[(size_t)k * ls4 + i];
        g[i] = s;
    }
    __syncthreads();
    int* steps = D.steps + (size_t)p * (kMaxNets + 1);
    const int t = steps[net] + 1;
    const float lr = a.stage == 0 ? a.critic_lr : a.actor_lr;
    const float total = adam_net(N.size, as_global(D.theta + off), as_global(D.m + off), as_global(D.v + off), as_global((const float*)(D.grad + off)),
                                 as_global(D.target + off), lr, 1e-8f, 0.9f, 0.999f, 0.f, 0.5f, t, a.tau, (lds_f)red_s);
    if (threadIdx.x != 0) return;
    steps[net] = t;
    const float* pt = D.part + part_offset(D, p, 0, 0);
    const int slot = a.stage == 0 ? (int)CEM_PART_CRITIC : CEM_PART_ACTOR + net;
    float l = 0.f;
    for (int k = 0; k < ns; ++k) l += pt[kPartFloats * k + slot];
    l /= (float)a.rows;
    float* out = D.cem_out + (size_t)p * kCemOut;
    float* st = D.stats + (size_t)p * ST_COUNT;
    const float kl = cem_kl(cem_c2_sum(D, p, ns), a.rows);
    if (a.stage == 0) {
        out[CEM_OUT_CRITIC_LOSS] = st[ST_CRITIC_LOSS] = l;
        out[CEM_OUT_CRITIC_NORM] = st[ST_CRITIC_GNORM] = total;
        out[CEM_OUT_KL] = kl;
        out[CEM_OUT_ROWS] = (float)a.rows;
        return;
    }
    if (net == cem_guided(D, p)) l += a.lambda * cem_delta(D, p) * kl;      // (:207 / :215)
    out[CEM_OUT_ACTOR_LOSS + 2 * net] = l;
    out[CEM_OUT_ACTOR_NORM + 2 * net] = total;
    if (net == CEM_ACTOR_1) { st[ST_ACTOR_LOSS] = l; st[ST_ACTOR_GNORM] = total; }
}

// ---------------------------------------------------------------------------------------- act
// frl_act on an ALGO_CEM_GD3PG engine: act_kernel's row load, the forward with the net's own hidden activation (tanh actors, the
// LeakyReLU critic), online or target, then act_epilogue.  grid = (row chunks, learners)
__global__ __launch_bounds__(256) void cem_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, rc = D.rc, r0 = blockIdx.x * rc;
    const NetDesc& N = D.net[a.net];
    const Lds S = carve(D, smem);
    const int nv = min(rc, a.n_rows - r0);
    g_cf theta = as_global((a.use_target ? D.target : D.theta) + (size_t)p * D.learner_stride + D.net_off[a.net]);
    const int K = a.in_dim, nout = N.L[N.n_layers - 1].n;
    g_cf in = as_global(a.in + ((size_t)p * a.n_rows + r0) * K);
    load_rows(S.xin, S.xp, rc, nv, in, 0, K, 0, K, N.L[0].k_pad);
    __syncthreads();
    mlp_fwd_rows(N, 0, N.n_layers, theta, S, a.mode == ACTM_TANH ? ACT_TANH : ACT_NONE, NoRowConsumer{}, NoRowConsumer{}, Leaky{});
    act_epilogue(D, a, N, theta, S.outb, S.op, nv, r0, p, nout);
}

}  // namespace frl
