// Envelope multi-objective DQN (ENVELOPE_MORL_file/ENVELOPE_DQN.py:204-255, after Yang et al. 2019) on the row-chunk skeleton of
// kernels_sacd.hip.  The Q-net takes [obs | w] (O + R columns) and returns one value per (action, objective): column a R + k.
// Launch chain (frl_api_envelope.inc):
//     [draw] -> envelope_weights_kernel -> envelope_grad_kernel -> reduce + Adam + soft update (kernels_update.hip)
// One learn() trains on N = B W rows: row j is sample idx[j % B] (the reference's tensor.repeat(W, 1)) under preference w[j / B]
// (np.repeat(B, axis = 0)).  A row chunk may straddle both a sample wrap and a weight boundary, so envelope_weights_kernel EXPANDS
// the B drawn ring rows to N entries of EngineDesc::idx (idx[j] = idx[j % B]) and gather_cols is used as it is; the preference of a
// row is looked up per row (j / B) when it is written into the R input columns behind the observation.
// Same grid, slabs and part[] as sacd_critic_kernel, so reduce / Adam / adam_publish serve the update unchanged.
#include <hip/hip_runtime.h>

#include "device/envelope.hpp"
#include "device/net.hpp"
#include "device/rng.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// ------------------------------------------------------------------------------------ weights
// One workgroup per learner.  (1) idx[j] = idx[j % B] for j in [B, N): the entries below B are only read, the ones from B up only
// written.  (2) a.draw_w: W preference vectors |n| / sum |n|, n ~ N(0, 1) from the engine's Philox stream (the reference's
// np.abs(randn) / L1 norm, :221-222); two passes over the same counters instead of R values in registers.
__global__ __launch_bounds__(256) void envelope_weights_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a) {
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x, B = a.batch, W = a.weight_num, NR = B * W, RD = D.reward_dim;
    g_i idx = (g_i)(D.idx + (size_t)p * D.batch_max);
    for (int j = B + threadIdx.x; j < NR; j += kWG) idx[j] = idx[j % B];
    if (!a.draw_w) return;
    const unsigned long long key = D.seed + 0x9E3779B97F4A7C15ull * (p + 1);
    g_f wts = as_global(D.env_w + (size_t)p * D.batch_max * RD);
    for (int wi = threadIdx.x; wi < W; wi += kWG) {
        float sum = 0.f;
        for (int k = 0; k < RD; k += 2) {
            float n0, n1;
            normal2(philox4x32_10(a.rng_counter, 0x7000u + (unsigned)(k >> 1), (unsigned)wi, key), n0, n1);
            sum += fabsf(n0);
            if (k + 1 < RD) sum += fabsf(n1);
        }
        for (int k = 0; k < RD; k += 2) {
            float n0, n1;
            normal2(philox4x32_10(a.rng_counter, 0x7000u + (unsigned)(k >> 1), (unsigned)wi, key), n0, n1);
            wts[(size_t)wi * RD + k] = fabsf(n0) / sum;
            if (k + 1 < RD) wts[(size_t)wi * RD + k + 1] = fabsf(n1) / sum;
        }
    }
}

// --------------------------------------------------------------------------------------- grad
// a' = argmax_a w . Q_online(s', w)[a, :] (the first maximum, as torch.max, :232-234); T = r + gamma Q_target(s', w)[a', :] (1 - done)
// (:235-240), an R-vector parked per row in abuf; Q = Q_online(s, w)[a, :] (:242);
//     loss = beta mean_j (w.Q - w.T)^2 + (1 - beta) mean_{j,k} (Q_k - T_k)^2 (:245-249)
// The head delta is non-zero only in the stored action's R columns: beta 2 (w.Q - w.T) w_k / N + (1 - beta) 2 (Q_k - T_k) / (N R).
// The row's preference stays in xin's columns [O, O + R) through all three forward passes (a gather rewrites the observation
// columns only), so every finalize step reads it from LDS.  Nothing per row stays in a register across the forward passes: a' waits
// in y, T in abuf.  Registers: tools/kernel_regs.py holds the kernel to its bound.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void envelope_grad_kernel(const EngineDesc* __restrict__ Dp, EnvelopeArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int p = U.p;
    const RecordDesc& R = D.rec;
    const NetDesc& N = D.net[0];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.batch, NR = B * a.weight_num;
    const RowWalk W = U.walk(NR);
    g_cf theta = U.theta(0);
    g_cf target = U.target(0);
    g_f slab = U.slab(0);
    g_cf ring = U.ring();
    g_cf wts = as_global(D.env_w + (size_t)p * D.batch_max * D.reward_dim);
    const int nl = N.n_layers;
    const int O = R.obs_dim[0], A = D.n_discrete, RD = D.reward_dim, k0pad = N.L[0].k_pad, npad = N.L[nl - 1].n_pad;
    const float invN = 1.f / (float)NR;
    const float c_env = a.beta * 2.f * invN, c_mse = (1.f - a.beta) * 2.f * invN / (float)RD;
    const float l_mse = (1.f - a.beta) / (float)RD;

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, r0 = c.r0, nv = c.nv;
    g_ci idx = c.idx;
    // ---- online net on [s' | w]: a' in y
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], O, 0);
    put_weights(S.xin, S.xp, rc, nv, wts, r0, B, RD, O);
    zero_cols(S.xin, S.xp, rc, O + RD, k0pad);
    FRL_PHASE(S);
    mlp_fwd_rows(N, 0, nl, theta, S, ACT_NONE, [&](int r) {
        if (r >= nv) return;
        lds_cf o = S.outb + r * S.op;
        lds_cf w = S.xin + r * S.xp + O;
        int best = 0;
        float bv = 0.f;
        for (int c = 0; c < A; ++c) {
            float v = 0.f;
            for (int k = 0; k < RD; ++k) v += o[c * RD + k] * w[k];
            if (c == 0 || v > bv) { bv = v; best = c; }
        }
        S.y[r] = (float)best;
    });
    // ---- target net on the same input: T parked in abuf
    mlp_fwd_rows(N, 0, nl, target, S, ACT_NONE, [&](int r) {
        if (r >= nv) return;
        lds_cf o = S.outb + r * S.op + (int)S.y[r] * RD;
        g_cf rec = ring + (size_t)idx[r] * R.stride;
        const float live = 1.f - rec[R.done_off];
        for (int k = 0; k < RD; ++k) S.abuf[r * S.ap + k] = rec[R.rew_off + k] + a.gamma * o[k] * live;
    });
    // ---- online net on [s | w] (the preference columns are still in place), the head delta, backward
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);
    FRL_PHASE(S);
    mlp_fwd_rows(N, 0, nl, theta, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        const int act = (r < nv) ? (int)ring[(size_t)idx[r] * R.stride + R.act_off[0]] : -1;     // the stored action index
        if (act >= 0 && act < A) {
            lds_cf w = S.xin + r * S.xp + O;
            lds_f t = S.abuf + r * S.ap;
            const int c0 = act * RD;
            float wq = 0.f, wt = 0.f, se = 0.f;
            for (int k = 0; k < RD; ++k) {
                const float q = o[c0 + k], e = q - t[k];
                wq += q * w[k];
                wt += t[k] * w[k];
                se += e * e;
                t[k] = e;                           // T is not needed again: the row's errors take its place
            }
            const float d = wq - wt;
            lossp += a.beta * d * d + l_mse * se;
            for (int c = 0; c < npad; ++c) {
                const int k = c - c0;
                o[c] = (k >= 0 && k < RD) ? c_env * d * w[k] + c_mse * t[k] : 0.f;
            }
        } else {
            for (int c = 0; c < npad; ++c) o[c] = 0.f;
        }
    });
    mlp_bwd(N, 0, nl, theta, slab, S, gs, false, 0, 0);
    }
    store_loss_part(U, S, lossp);
}
}  // namespace frl
