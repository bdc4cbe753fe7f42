// Envelope multi-objective DDPG (ENVELOPE_MORL_file/ENVELOPE_DDPG.py:254-320) on the row-chunk skeleton: the critic-then-actor shape
// of kernels_critic.hip / kernels_actor.hip over the N = B W rows of kernels_envelope.hip (row j: sample idx[j % B] under preference
// w[j / B]; envelope_weights_kernel expands the rows and draws the preferences).
// Launch chain (frl_api_envelope_ddpg.inc):
//     [draw] -> envelope_weights_kernel -> envelope_ddpg_critic_kernel -> reduce + clip + Adam + soft update (critic)
//            -> envelope_ddpg_actor_kernel -> reduce + clip + Adam + soft update (actor)
// Net 0 is the actor on [obs | w] (O + R columns, tanh head of A columns), net 1 the critic on [obs | act | w] (O + A + R columns,
// linear head of R columns).  The preference sits at column O in the actor's input and at column O + A in the critic's, so it is
// written once per net layout of a chunk: the gathers in between rewrite the columns in front of it only.
// Same grid, slabs and part[] as envelope_grad_kernel, so reduce / Adam / adam_publish serve both updates unchanged.
#include <hip/hip_runtime.h>

#include "device/envelope.hpp"
#include "device/net.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// ------------------------------------------------------------------------------------- critic
// a' = actor(s', w) of the ONLINE actor (:284); T = r + gamma critic_target(s', a', w) (1 - done) (:285-287), an R-vector parked
// per row in abuf; Q = critic(s, a, w) (:290);
//     loss = beta mean_j (w.Q - w.T)^2 + (1 - beta) mean_{j,k} (Q_k - T_k)^2 (:293-297)
// Head delta of row j, column k: beta 2 (w.Q - w.T) w_k / N + (1 - beta) 2 (Q_k - T_k) / (N R); zero in the rows past the
// chunk's valid ones and in the padded columns.  Nothing per row stays in a register across the passes: a' goes straight into the
// critic's input row, T waits in abuf.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void envelope_ddpg_critic_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int p = U.p;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[0];
    const NetDesc& NC = D.net[1];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.batch, NR = B * a.weight_num;
    const RowWalk W = U.walk(NR);
    g_cf thA = U.theta(0);
    g_cf thC = U.theta(1);
    g_cf tgC = U.target(1);
    g_f slab = U.slab(1);
    g_cf ring = U.ring();
    g_cf wts = as_global(D.env_w + (size_t)p * D.batch_max * D.reward_dim);
    const int O = R.obs_dim[0], A = R.act_dim[0], RD = D.reward_dim;
    const int ka0 = NA.L[0].k_pad, kc0 = NC.L[0].k_pad, npad = NC.L[NC.n_layers - 1].n_pad;

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, r0 = c.r0, nv = c.nv;
    g_ci idx = c.idx;
    // ---- online actor on [s' | w]: a' straight into the critic's input row (the first layer has read xin by then)
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], O, 0);
    put_weights(S.xin, S.xp, rc, nv, wts, r0, B, RD, O);
    zero_cols(S.xin, S.xp, rc, O + RD, ka0);
    FRL_PHASE(S);
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_TANH, [&](int r) {
        for (int c = 0; c < A; ++c) S.xin[r * S.xp + O + c] = S.outb[r * S.op + c];
    });
    // ---- critic target on [s' | a' | w]: T parked in abuf
    put_weights(S.xin, S.xp, rc, nv, wts, r0, B, RD, O + A);
    zero_cols(S.xin, S.xp, rc, O + A + RD, kc0);
    FRL_PHASE(S);
    mlp_fwd_rows(NC, 0, NC.n_layers, tgC, S, ACT_NONE, [&](int r) {
        if (r >= nv) return;
        lds_cf o = S.outb + r * S.op;
        g_cf rec = ring + (size_t)idx[r] * R.stride;
        const float live = 1.f - rec[R.done_off];
        for (int k = 0; k < RD; ++k) S.abuf[r * S.ap + k] = rec[R.rew_off + k] + a.gamma * o[k] * live;
    });
    // ---- critic on [s | a | w] (obs and the stored action are adjacent in a record; the preference columns are still in place),
    //      the head delta, backward
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O + A, 0);
    FRL_PHASE(S);
    mlp_fwd_rows(NC, 0, NC.n_layers, thC, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        if (r < nv) {
            lds_cf w = S.xin + r * S.xp + O + A;
            lds_f t = S.abuf + r * S.ap;
            float wq = 0.f, wt = 0.f, se = 0.f;
            for (int k = 0; k < RD; ++k) {
                const float q = o[k], e = q - t[k];
                wq += q * w[k];
                wt += t[k] * w[k];
                se += e * e;
                t[k] = e;                           // T is not needed again: the row's errors take its place
            }
            const float d = wq - wt;
            // (the coefficients are formed here, not ahead of the chunk loop: held across the passes they cost five more spilled VGPRs)
            const float invN = 1.f / (float)NR;
            const float c_env = a.beta * 2.f * invN, c_mse = (1.f - a.beta) * 2.f * invN / (float)RD;
            lossp += a.beta * d * d + (1.f - a.beta) / (float)RD * se;
            for (int c = 0; c < npad; ++c) o[c] = c < RD ? c_env * d * w[c] + c_mse * t[c] : 0.f;
        } else {
            for (int c = 0; c < npad; ++c) o[c] = 0.f;
        }
    });
    mlp_bwd(NC, 0, NC.n_layers, thC, slab, S, gs, false, 0, 0);
    }
    store_loss_part(U, S, lossp);
}

// -------------------------------------------------------------------------------------- actor
// a = actor(s, w); loss = -mean_{j,k} critic(s, a, w)_k through the critic just updated (:302-303; the objectives are NOT weighted
// by w): the critic's head delta is -1 / (N R) in each of its R columns, a dX-only backward reaches the action column tiles, then
// tanh' and the actor's backward.  The shape of ac_actor_kernel with one critic head of R columns.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void envelope_ddpg_actor_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int p = U.p;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[0];
    const NetDesc& NC = D.net[1];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.batch, NR = B * a.weight_num;
    const RowWalk W = U.walk(NR);
    g_cf thA = U.theta(0);
    g_cf thC = U.theta(1);
    g_f slab = U.slab(0);
    g_cf ring = U.ring();
    g_cf wts = as_global(D.env_w + (size_t)p * D.batch_max * D.reward_dim);
    const int O = R.obs_dim[0], A = R.act_dim[0], RD = D.reward_dim;
    const int ka0 = NA.L[0].k_pad, kc0 = NC.L[0].k_pad;
    const int ncpad = NC.L[NC.n_layers - 1].n_pad, napad = NA.L[NA.n_layers - 1].n_pad;
    const int ct0 = O / 16, ct1 = (O + A + 15) / 16;            // the action's column tiles of the critic's input
    const float dq = -1.f / ((float)NR * (float)RD), invR = 1.f / (float)RD;
    // the actor's hidden activations park in HBM over the critic pass, as in ac_actor_kernel
    FRL_GLB f32x4* spill = U.spill();

    float alossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, r0 = c.r0, nv = c.nv;
    g_ci idx = c.idx;
    // ---- a = actor([s | w]): kept in abuf for tanh', and written into the critic's input row
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);
    put_weights(S.xin, S.xp, rc, nv, wts, r0, B, RD, O);
    zero_cols(S.xin, S.xp, rc, O + RD, ka0);
    FRL_PHASE(S);
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_TANH, [&](int r) {
        for (int c = 0; c < A; ++c) {
            const float av = S.outb[r * S.op + c];
            S.abuf[r * S.ap + c] = av;
            S.xin[r * S.xp + O + c] = av;
        }
    }, [&]() { park_hidden(S, spill); });
    // ---- critic on [s | a | w]: the sum of its R outputs, the constant head delta, dX into the action column tiles
    put_weights(S.xin, S.xp, rc, nv, wts, r0, B, RD, O + A);
    zero_cols(S.xin, S.xp, rc, O + A + RD, kc0);
    FRL_PHASE(S);
    mlp_fwd_rows(NC, 0, NC.n_layers, thC, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        const bool live = r < nv;
        float qs = 0.f;
        for (int c = 0; c < ncpad; ++c) {
            if (live && c < RD) qs += o[c];
            o[c] = (live && c < RD) ? dq : 0.f;
        }
        alossp -= qs * invR;
    });
    mlp_bwd(NC, 0, NC.n_layers, thC, nullptr, S, GS_ADD, true, ct0, ct1);
    for (int e = threadIdx.x; e < rc * A; e += kWG) {
        const int r = e / A, c = e - r * A;
        S.dabuf[r * S.ap + c] = S.xin[r * S.xp + O + c];
    }
    FRL_PHASE(S);
    // ---- the actor's activations back from HBM (same thread, same addresses as the spill), its input back in xin
    restore_hidden(S, spill);
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);      // (the critic's dX landed on xin)
    put_weights(S.xin, S.xp, rc, nv, wts, r0, B, RD, O);
    zero_cols(S.xin, S.xp, rc, O + RD, ka0);
    // the head delta in the same phase: it reads dabuf / abuf and writes outb, none of which the reload above touches
    for (int e = threadIdx.x; e < rc * napad; e += kWG) {
        const int r = e / napad, c = e - r * napad;
        S.outb[r * S.op + c] = (r < nv && c < A) ? tanh_delta(S.dabuf[r * S.ap + c], S.abuf[r * S.ap + c]) : 0.f;
    }
    FRL_PHASE(S);
    mlp_bwd(NA, 0, NA.n_layers, thA, slab, S, gs, false, 0, 0);
    }
    store_loss_part(U, S, alossp);
}
}  // namespace frl
