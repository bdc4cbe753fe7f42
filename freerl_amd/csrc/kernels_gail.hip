// GAIL's discriminator (GAIL_file/GAIL.py:17-120) on the row-chunk skeleton of kernels_envelope.hip: one net (index 0)
// [obs | act] -> H -> H -> 1 with LeakyReLU (or ReLU) hidden layers, no target.  The ring holds the EXPERT rows.
// Launch chain (frl_api_gail.inc):
//     [gail_draw_kernel] -> gail_disc_kernel -> reduce + Adam (kernels_update.hip, no clip, no soft update) -> gail_stats_kernel
// One trian_D() trains on E + N rows: row j < E is expert ring row idx[j], row E + i policy row i of the call's staged rows; a row
// chunk may hold both kinds.  gp = 0: sigmoid + F.binary_cross_entropy per side (:107-109); gp = 1: 0.5 x BCE-with-logits per side plus
// gp_weight x mean_e ||dl/dx||^2 (:84-98), the penalty's gradient in the closed form of device/gail.hpp.
// Same grid, slabs and reduce / Adam launches as envelope_grad_kernel; the seven partial sums of a workgroup go to gail_part.
// gail_forward_kernel: the forward alone — logits (frl_act with FRL_ACT_RAW), or compute_reward (:62-73).
#include <hip/hip_runtime.h>

#include "device/gail.hpp"
#include "device/rng.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// ------------------------------------------------------------------------------------- draw
// n_expert ring rows per learner WITH replacement (InfiniteUniformSampler's torch.randint, GAIL_utils.py:51-56) from the engine's
// Philox stream: one independent draw per entry, no duplicate check.
__global__ __launch_bounds__(256) void gail_draw_kernel(const EngineDesc* __restrict__ Dp, GailArgs a) {
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x;
    g_i idx = (g_i)(D.idx + (size_t)p * D.batch_max);
    const unsigned long long key = D.seed + 0x9E3779B97F4A7C15ull * (p + 1);
    for (int i = threadIdx.x; i < a.n_expert; i += kWG)
        idx[i] = (int)uniform_index(philox4x32_10(a.rng_counter, 0xA000u, (unsigned)i, key), (unsigned)a.size);
}

// ------------------------------------------------------------------------------------- disc
// Per row chunk: gather -> forward (rowf: the row's loss terms and BCE head delta; allf: the slope bits) -> mlp_bwd into the slab.
// gp: the unit backward is rebuilt from the slope bits after the BCE backward has overwritten the activations — u2 = m2 (.) w3 needs
// no matrix product, h1 takes +-1 so that linear_bwd_dx's act_grad finds the slopes — with head delta 1 on the expert rows and 0
// elsewhere, which makes g, t0 and with them s1, s2 vanish on policy and invalid rows: no second code path.  Then
//     g -> xin, penalty partial, t0 in place | dW1 += u1 (x) t0 | s1 -> h1 | dW2 += u2 (x) s1 | s2 -> h2 | dw3 += s2
// The three GS_ADD products re-read what the BCE pass of the same chunk stored: same function, same shape, so the same thread
// owns an element both times (a head that went through head_bwd: head_tangent_dw) — hence GS_STORE, not GS_STREAM, for the first chunk.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void gail_disc_kernel(const EngineDesc* __restrict__ Dp, GailArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int p = U.p;
    const RecordDesc& R = D.rec;
    const NetDesc& N = D.net[0];
    const Lds S = carve(D, smem);
    const int rc = D.rc, E = a.n_expert, NR = E + a.n_policy;
    const RowWalk W = U.walk(NR, a.gp != 0);
    g_cf theta = U.theta(0);
    g_f slab = U.slab(0);
    g_cf ring = U.ring();
    const int IN = R.obs_dim[0] + R.act_dim[0], k0pad = N.L[0].k_pad, npad = N.L[2].n_pad, H = N.L[0].n;
    g_cf rows = as_global(D.gail_rows + (size_t)p * D.batch_max * IN);
    g_ci idx = U.idx(0);                                            // (gail_gather indexes from the call's first row)
    lds_u bits1 = (lds_u)S.abuf, bits2 = (lds_u)S.dabuf;            // the slope bits of h1 / h2, S.ap words per row
    const float slope = N.hidden_act == ACT_LEAKY_RELU ? kLeakySlope : 0.f;
    const bool fuse = head_fusable(N, 0, 3);

    float sum[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};              // GailPart, per thread (= per row of a chunk)
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, r0 = c.r0;
    gail_gather(S.xin, S.xp, rc, r0, E, NR, idx, ring, R.stride, R.obs_off[0], rows, IN);
    zero_cols(S.xin, S.xp, rc, IN, k0pad);
    FRL_PHASE(S);
    mlp_fwd_rows(N, 0, 3, theta, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        const int j = r0 + r;
        const float l = o[0];
        float d = 0.f;
        if (j < NR) {
            const bool ex = j < E;
            const float inv = 1.f / (float)(ex ? E : a.n_policy), t = ex ? 1.f : 0.f;
            const float pr = sigmoid_f(l);
            float bce;
            if (a.gp) {
                // F.binary_cross_entropy_with_logits, mean, x 0.5 (:84-86): d/dl = 0.5 (sigmoid(l) - t) / rows
                bce = softplus_f(ex ? -l : l);
                d = 0.5f * inv * (pr - t);
            } else {
                // F.binary_cross_entropy on sigmoid(l) (:107-108): the log clamped at -100; its backward divides by
                // max(p (1 - p), 1e-12), sigmoid's multiplies by p (1 - p)
                bce = -fmaxf(logf(ex ? pr : 1.f - pr), -100.f);
                const float q = (1.f - pr) * pr;
                d = (inv * (pr - t) / fmaxf(q, 1e-12f)) * q;
            }
            // (constant slots: a slot picked by `ex` would put the sums in scratch)
            sum[GP_BCE_E] += ex ? bce : 0.f;   sum[GP_BCE_P] += ex ? 0.f : bce;
            sum[GP_PROB_E] += ex ? pr : 0.f;   sum[GP_PROB_P] += ex ? 0.f : pr;
            sum[GP_LOGIT_E] += ex ? l : 0.f;   sum[GP_LOGIT_P] += ex ? 0.f : l;
        }
        for (int c = 0; c < npad; ++c) o[c] = c == 0 ? d : 0.f;
    }, [&]() {
        if (!a.gp) return;
        slope_pack(S.h1, S.hp, H, rc, bits1, S.ap);
        slope_pack(S.h2, S.hp, H, rc, bits2, S.ap);
    }, std::true_type{});
    mlp_bwd(N, 0, 3, theta, slab, S, gs, false, 0, 0, std::true_type{});
    if (a.gp) {
        // ---- the unit backward from the slope bits: h2 = u2 (expert rows; 0 elsewhere), h1 = +-1, then u1 and g = dl/dx
        g_cf w3 = theta + N.L[2].w_off;                           // Wk[k_pad][16]: column 0
        for (int e = threadIdx.x; e < rc * H; e += kWG) {
            const int r = e / H, k = e - r * H;
            const float m2 = slope_bit(bits2, S.ap, r, k) ? 1.f : slope;
            S.h2[r * S.hp + k] = (r0 + r < E) ? m2 * w3[k * 16] : 0.f;
            S.h1[r * S.hp + k] = slope_bit(bits1, S.ap, r, k) ? 1.f : -1.f;
        }
        FRL_PHASE(S);
        linear_bwd_dx<true>(N.L[1], theta, S.h2, S.hp, S.h1, S.hp, N.hidden_act, rc, 0, N.L[1].k_pad / 16);
        FRL_PHASE(S);
        linear_bwd_dx(N.L[0], theta, S.h1, S.hp, S.xin, S.xp, ACT_NONE, rc, 0, k0pad / 16);
        FRL_PHASE(S);
        // ---- the penalty's partial sum and the tangent t0 = 2 c g / E, in place (one thread per row)
        if ((int)threadIdx.x < rc) {
            lds_f x = S.xin + threadIdx.x * S.xp;
            const float ts = 2.f * a.gp_weight / (float)E;
            float ss = 0.f;
            for (int c = 0; c < k0pad; ++c) {
                const float g = c < IN ? x[c] : 0.f;
                ss += g * g;
                x[c] = ts * g;
            }
            sum[GP_PEN] += ss;
        }
        FRL_PHASE(S);
        linear_bwd_dw(N.L[0], slab, S.h1, S.hp, S.xin, S.xp, rc, GS_ADD, false);      // dW1 += u1 (x) t0
        FRL_PHASE(S);
        tangent_fwd(N.L[0], theta, S.xin, S.xp, S.h1, S.hp, rc, bits1, S.ap, slope);   // s1 over u1
        FRL_PHASE(S);
        linear_bwd_dw(N.L[1], slab, S.h2, S.hp, S.h1, S.hp, rc, GS_ADD, false);       // dW2 += u2 (x) s1
        FRL_PHASE(S);
        tangent_fwd(N.L[1], theta, S.h1, S.hp, S.h2, S.hp, rc, bits2, S.ap, slope);    // s2 over u2
        if (!fuse)
            for (int e = threadIdx.x; e < rc * npad; e += kWG) S.outb[(e / npad) * S.op + e % npad] = (e % npad) == 0 ? 1.f : 0.f;
        FRL_PHASE(S);
        if (fuse) head_tangent_dw(N.L[2], slab, S.h2, S.hp, rc);                       // dw3 += s2
        else linear_bwd_dw(N.L[2], slab, S.outb, S.op, S.h2, S.hp, rc, GS_ADD, false);
    }
    }
    g_f part = as_global(D.gail_part + unit_slice_index(D, p, 0, U.sl) * GP_COUNT);
    for (int i = 0; i < 7; ++i) {
        const float s = block_sum(sum[i], S.red);
        if (threadIdx.x == 0) part[i] = s;
    }
}

// ------------------------------------------------------------------------------------ stats
// After the Adam launch: a learner's seven sums over its workgroups in slab order -> what trian_D returns (:100-120), the penalty
// mean and the gradient norm the Adam launch published.
__global__ __launch_bounds__(256) void gail_stats_kernel(const EngineDesc* __restrict__ Dp, GailArgs a, int ns) {
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x * kWG + threadIdx.x;
    if (p >= D.P) return;
    float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < ns; ++k)
        for (int i = 0; i < 7; ++i) s[i] += D.gail_part[unit_slice_index(D, p, 0, k) * GP_COUNT + i];
    const float invE = 1.f / (float)a.n_expert, invN = 1.f / (float)a.n_policy;
    float* o = D.gail_out + (size_t)p * 8;
    float* st = D.stats + (size_t)p * ST_COUNT;
    const float pen = a.gp ? s[GP_PEN] * invE : 0.f;
    const float bce = s[GP_BCE_E] * invE + s[GP_BCE_P] * invN;
    o[GO_LOSS] = a.gp ? 0.5f * bce + a.gp_weight * pen : bce;
    o[GO_PROB_E] = s[GP_PROB_E] * invE;
    o[GO_PROB_P] = s[GP_PROB_P] * invN;
    o[GO_WDIS] = a.gp ? s[GP_LOGIT_E] * invE - s[GP_LOGIT_P] * invN : 0.f;
    o[GO_PEN] = pen;
    o[GO_GNORM] = st[ST_ACTOR_GNORM];
    st[ST_ACTOR_LOSS] = o[GO_LOSS];
}

// ---------------------------------------------------------------------------------- forward
// grid = (row chunks, learners) over n_rows dense rows per learner.  mode 0: logits; 1: -log(1 - sigmoid(l) + 1e-8) (:71-72);
// 2: 2 x -log(max(1 - 1 / (1 + exp(-l)), 1e-4)) (:65-69) — fp32, in the reference's order of operations.
__global__ __launch_bounds__(256) void gail_forward_kernel(const EngineDesc* __restrict__ Dp, int mode, int n_rows, const float* __restrict__ in,
                                                           float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, rc = D.rc, r0 = blockIdx.x * rc, nv = min(rc, n_rows - r0);
    const NetDesc& N = D.net[0];
    const Lds S = carve(D, smem);
    g_cf theta = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[0]);
    const int IN = N.L[0].k, k0pad = N.L[0].k_pad;
    g_cf x = as_global(in + ((size_t)p * n_rows + r0) * IN);
    load_rows(S.xin, S.xp, rc, nv, x, 0, IN, 0, IN, k0pad);
    FRL_PHASE(S);
    g_f y = as_global(out + (size_t)p * n_rows + r0);
    mlp_fwd_rows(N, 0, 3, theta, S, ACT_NONE, [&](int r) {
        if (r >= nv) return;
        const float l = S.outb[r * S.op];
        float v = l;
        if (mode == 1) v = -logf(1.f - sigmoid_f(l) + 1e-8f);
        if (mode == 2) {
            const float prob = 1.f / (1.f + expf(-l));
            v = -logf(fmaxf(1.f - prob, 0.0001f)) * 2.f;
        }
        y[r] = v;
    }, NoRowConsumer{}, std::true_type{});
}
}  // namespace frl
