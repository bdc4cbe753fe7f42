// Gradient kernels of discrete SAC (SAC_file/SAC_add_discrete.py:288-348, the `hands_on` branch) on the row-chunk skeleton of
// kernels_critic.hip / kernels_actor.hip.  Launch chain (frl_api.hip, launch_learn_stage):
//     [draw] -> [obsnorm] -> sacd_critic_kernel -> Adam(critic) + soft update -> sacd_actor_kernel -> Adam(actor) + soft update + alpha
// Same grid, slabs and part[] as the continuous kernels, so reduce / Adam / adam_publish serve them unchanged.
#include <hip/hip_runtime.h>

#include "device/net.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// torch.softmax of one row's logits o[0:A) into p[0:A) (max-subtracted, scaled by the reciprocal of the sum);
// returns H = -sum p * log(p + 1e-8) (SAC_add_discrete.py:297,326)
__device__ __forceinline__ float sacd_softmax(lds_cf o, lds_f p, int A) {
    float mx = o[0];
    for (int j = 1; j < A; ++j) mx = fmaxf(mx, o[j]);
    float sum = 0.f;
    for (int j = 0; j < A; ++j) {
        const float ex = expf(o[j] - mx);
        p[j] = ex;
        sum += ex;
    }
    const float inv = 1.f / sum;
    float ent = 0.f;
    for (int j = 0; j < A; ++j) {
        const float pj = p[j] * inv;
        p[j] = pj;
        ent -= pj * logf(pj + 1e-8f);
    }
    return ent;
}

// ------------------------------------------------------------------------------------- critic
// y = r + gamma (1 - d) (sum_a p'_a min(V1'_a, V2'_a) + alpha H(p')), p' = softmax(actor(s')) of the ONLINE actor, V' from the
// target critic (:294-306); loss = mse(V1(s)[a], y) + mse(V2(s)[a], y) (:310-314); both heads' backward into the slab.
// Registers: 256 VGPRs with 9 spilled (tools/asm_spills.py): the Lds carve's pointers / pitches and the chunk loop's bounds, stored
// once at entry and reloaded at the start of a forward / backward pass (net.hpp:413, 469) or of a row chunk — about twenty
// scratch loads per row chunk, none inside an MFMA loop.  tools/kernel_regs.py holds the count to this bound.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void sacd_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int p = U.p;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[0];
    const NetDesc& NC = D.net[1];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.batch;
    const RowWalk W = U.walk(B);
    g_cf thA = U.theta(0);
    g_cf thC = U.theta(1);
    g_cf tgC = U.target(1);
    g_f slab = U.slab(1);
    g_cf ring = U.ring();
    const int ql = NC.n_layers / NC.heads;
    const int O = R.obs_dim[0], A = D.n_discrete, kc0 = NC.L[0].k_pad;
    const float alpha = D.alpha[p * 4 + 3];
    const float invB = 1.f / (float)B;
    g_cf bn = D.obs_norm_on ? as_global(D.obsnorm + (size_t)p * D.obsnorm_w) : nullptr;
    FRL_PHASE_INIT(S);

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, nv = c.nv;
    g_ci idx = c.idx;
    // ---- p' = actor(s') and H(p'): softmax in the finalize phase, p' parked in abuf, H(p') in y (nothing per row stays in a
    // register across the forward passes: each finalize step reads what it needs from LDS or the ring)
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], O, 0);
    zero_cols(S.xin, S.xp, rc, O, kc0);
    if (bn) { lds_barrier(); normalize_cols(S.xin, S.xp, nv, 0, O, bn, O); }
    FRL_PHASE(S);
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_NONE, [&](int r) {
        S.y[r] = sacd_softmax(S.outb + r * S.op, S.abuf + r * S.ap, A);
    });
    // ---- target critic on s' (xin still holds it): V1' parked in dabuf, then sum_a p'_a min(V1'_a, V2'_a)
    mlp_fwd_rows(NC, 0, ql, tgC, S, ACT_NONE, [&](int r) {
        for (int c = 0; c < A; ++c) S.dabuf[r * S.ap + c] = S.outb[r * S.op + c];
    });
    mlp_fwd_rows(NC, ql, ql, tgC, S, ACT_NONE, [&](int r) {
        if (r >= nv) return;
        float v = 0.f;
        for (int c = 0; c < A; ++c) v += S.abuf[r * S.ap + c] * fminf(S.dabuf[r * S.ap + c], S.outb[r * S.op + c]);
        g_cf rec = ring + (size_t)idx[r] * R.stride;
        const float rew = rec[R.rew_off], done = rec[R.done_off];
        S.y[r] = rew + a.gamma * (1.f - done) * (v + alpha * S.y[r]);
    });
    // ---- online critic on s: both heads read the same rows (nothing in between writes xin)
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);
    zero_cols(S.xin, S.xp, rc, O, kc0);
    if (bn) { lds_barrier(); normalize_cols(S.xin, S.xp, nv, 0, O, bn, O); }
    FRL_PHASE(S);
    for (int h = 0; h < 2; ++h) {
        const int npad = NC.L[h * ql + ql - 1].n_pad;
        mlp_fwd_rows(NC, h * ql, ql, thC, S, ACT_NONE, [&](int r) {      // delta only at the stored action's column: 2 (Q_h - y) / B
            lds_f o = S.outb + r * S.op;
            float d = 0.f;
            int col = -1;
            const int act = (r < nv) ? (int)ring[(size_t)idx[r] * R.stride + R.act_off[0]] : -1;     // the stored action index
            if (act >= 0 && act < A) {
                float lrow, grow;
                td_loss_row(a, o[act] - S.y[r], lrow, grow);
                d = grow * invB;
                col = act;
                lossp += lrow;
            }
            for (int c = 0; c < npad; ++c) o[c] = (c == col) ? d : 0.f;
        });
        mlp_bwd(NC, h * ql, ql, thC, slab, S, gs, false, 0, 0);
    }
    }
    FRL_PHASE_DUMP(S, 10);
    store_loss_part(U, S, lossp);
}

// -------------------------------------------------------------------------------------- actor
// With the UPDATED critic (:319-330): p = softmax(actor(s)), m = min(V1(s), V2(s)), loss = mean(-sum p m - alpha H(p)).
// The gradient reaches the actor only (the critic's share of the reference's backward is cleared by the next zero_grad):
//     g_j = (-m_j + alpha (log(p_j + 1e-8) + p_j / (p_j + 1e-8))) / B,   dz_j = p_j (g_j - sum_k p_k g_k)
// The critic runs first, so the actor's hidden activations are still in h1 / h2 for its backward: no spill, no second forward.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void sacd_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int p = U.p;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[0];
    const NetDesc& NC = D.net[1];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.batch;
    const RowWalk W = U.walk(B);
    g_cf thA = U.theta(0);
    g_cf thC = U.theta(1);
    g_f slab = U.slab(0);
    g_cf ring = U.ring();
    const int ql = NC.n_layers / NC.heads;
    const int O = R.obs_dim[0], A = D.n_discrete, kc0 = NA.L[0].k_pad;
    const int napad = NA.L[NA.n_layers - 1].n_pad;
    const float alpha = D.alpha[p * 4 + 3];
    const float invB = 1.f / (float)B;
    g_cf bn = D.obs_norm_on ? as_global(D.obsnorm + (size_t)p * D.obsnorm_w) : nullptr;
    FRL_PHASE_INIT(S);

    float alossp = 0.f, entp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, nv = c.nv;
    g_ci idx = c.idx;
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);
    zero_cols(S.xin, S.xp, rc, O, kc0);
    if (bn) { lds_barrier(); normalize_cols(S.xin, S.xp, nv, 0, O, bn, O); }
    FRL_PHASE(S);
    // ---- m = min(V1(s), V2(s)) in dabuf (forward only)
    mlp_fwd_rows(NC, 0, ql, thC, S, ACT_NONE, [&](int r) {
        for (int c = 0; c < A; ++c) S.dabuf[r * S.ap + c] = S.outb[r * S.op + c];
    });
    mlp_fwd_rows(NC, ql, ql, thC, S, ACT_NONE, [&](int r) {
        for (int c = 0; c < A; ++c) S.dabuf[r * S.ap + c] = fminf(S.dabuf[r * S.ap + c], S.outb[r * S.op + c]);
    });
    // ---- actor forward on the same rows; the row's loss, entropy and logit delta in the finalize phase
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        if (r < nv) {
            lds_f pr = S.abuf + r * S.ap;
            lds_f g = S.dabuf + r * S.ap;           // m, overwritten by g once read
            const float ent = sacd_softmax(o, pr, A);
            float q = 0.f, pg = 0.f;
            for (int c = 0; c < A; ++c) {
                const float pc = pr[c], m = g[c];
                q += pc * m;
                const float gc = (-m + alpha * (logf(pc + 1e-8f) + pc / (pc + 1e-8f))) * invB;
                g[c] = gc;
                pg += pc * gc;
            }
            for (int c = 0; c < napad; ++c) o[c] = (c < A) ? pr[c] * (g[c] - pg) : 0.f;
            alossp += -q - alpha * ent;
            entp += ent;
        } else {
            for (int c = 0; c < napad; ++c) o[c] = 0.f;
        }
    });
    mlp_bwd(NA, 0, NA.n_layers, thA, slab, S, gs, false, 0, 0);
    }
    FRL_PHASE_DUMP(S, 11);
    const float la = block_sum(alossp, S.red);
    const float le = block_sum(entp, S.red);
    store_loss_parts(U, la, le);
}
}  // namespace frl
