// MAPPO / IPPO / HAPPO device code (MAPPO_file/MAPPO.py, IPPO.py, HAPPO.py): the normalised forward and backward of one row chunk, the
// clipped surrogate of a row over one or n_agents advantage columns, and the K_epochs x minibatch steps of one net that kernels_mappo,
// _mappo_mask, _mappo_state and _happo all run; and the critic's second input segment (MAPPO_for_mask_action_state.py) for
// kernels_mappo_state.hip.  The head arithmetic itself — the surrogate term, the Normal and the (masked) categorical head, the
// critic's row, the advantage normalisation — is device/onpolicy.hpp's, shared with the PPO and GAIL-PPO kernels.
//
// Forward: [feature_norm] -> l1 -> ReLU -> [LN] -> l2 -> ReLU -> [LN] -> head, both norms F.layer_norm without affine part, biased
// variance, eps 1e-5.  Without LayerNorm this is device/net.hpp's mlp_fwd / mlp_bwd as they are (feature_norm rewrites xin only and
// needs no backward: it is the input).  With it a hidden layer keeps its NORMALISED row in h1 / h2 (the next layer's input and the
// xhat of the LayerNorm backward), one rstd per row, and its ReLU mask as one bit per unit; the backward of a layer is
//     dn = dY W  (plain)  ->  da = rstd (dn - mean(dn) - xhat mean(dn xhat))  ->  dz = da where the unit was positive
// with dn written to a third hidden buffer (dbuf) so that xhat survives until the row's two means are taken.  One wave walks a row and
// both means are a fixed butterfly over its 64 lanes: the same bits on every run.
#pragma once
#include "onpolicy.hpp"
#include "../kernels.h"

namespace frl {

constexpr float kLnEps = 1e-5f;          // F.layer_norm's default

struct MappoLds {
    lds_f dbuf;                  // [rc][hp] d loss / d (normalised row), then the layer's delta
    lds_f rstd;                  // [2][rc]
    FRL_LDS unsigned* mask;      // [2][rc][kMappoMaskWords]
};

__device__ __forceinline__ MappoLds carve_mappo(const Lds& S) {
    MappoLds X;
    lds_f p = S.red + 8;
    X.dbuf = p; p += S.rc * S.hp;
    X.rstd = p; p += 2 * S.rc;
    X.mask = (FRL_LDS unsigned*)p;
    return X;
}

// x <- (x - mean) / sqrt(var + eps) over the first n columns of every row; one wave per row.  bits != nullptr: bit c of the row's mask
// = (x[c] > 0) BEFORE the normalisation (the ReLU that produced x passes gradient there); rs != nullptr: the row's rstd.
__device__ __forceinline__ void ln_rows(lds_f X, int ldx, int n, int rc, lds_f rs, FRL_LDS unsigned* bits) {
    const int l = lane_id(), w = wave_id();
    const float inv = 1.f / (float)n;
    for (int r = w; r < rc; r += kWaves) {
        lds_f x = X + r * ldx;
        float s = 0.f;
        for (int c = l; c < n; c += 64) s += x[c];
        const float mean = wave_sum(s) * inv;
        float q = 0.f;
        for (int c = l; c < n; c += 64) { const float d = x[c] - mean; q += d * d; }
        const float rstd = 1.f / sqrtf(wave_sum(q) * inv + kLnEps);
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int c = c0 + l;
            const float v = c < n ? x[c] : 0.f;
            if (bits) {
                const unsigned long long b = __ballot(v > 0.f);
                if (l == 0) { bits[r * kMappoMaskWords + (c0 >> 5)] = (unsigned)b; bits[r * kMappoMaskWords + (c0 >> 5) + 1] = (unsigned)(b >> 32); }
            }
            if (c < n) x[c] = (v - mean) * rstd;
        }
        if (rs && l == 0) rs[r] = rstd;
    }
}

// dY (the gradient at the normalised row) -> the layer's delta, in place: through F.layer_norm, then the ReLU mask
__device__ __forceinline__ void ln_bwd_rows(lds_f dY, lds_cf Xhat, int ld, int n, int rc, lds_cf rs, const FRL_LDS unsigned* bits) {
    const int l = lane_id(), w = wave_id();
    const float inv = 1.f / (float)n;
    for (int r = w; r < rc; r += kWaves) {
        lds_f dy = dY + r * ld;
        lds_cf xh = Xhat + r * ld;
        float s1 = 0.f, s2 = 0.f;
        for (int c = l; c < n; c += 64) { const float g = dy[c]; s1 += g; s2 += g * xh[c]; }
        const float m1 = wave_sum(s1) * inv, m2 = wave_sum(s2) * inv, rstd = rs[r];
        for (int c = l; c < n; c += 64) {
            const bool open = (bits[r * kMappoMaskWords + (c >> 5)] >> (c & 31)) & 1u;
            dy[c] = open ? rstd * ((dy[c] - m1) - xh[c] * m2) : 0.f;
        }
    }
}

// Forward of a three-layer net on the chunk in xin (kin real input columns).  Ends with a barrier; the head's rows are in outb.
__device__ __forceinline__ void mappo_fwd(const EngineDesc& D, const NetDesc& N, g_cf theta, const Lds& S, const MappoLds& X, int kin,
                                          int out_act) {
    if (D.feature_norm) {
        ln_rows(S.xin, S.xp, kin, S.rc, nullptr, nullptr);
        FRL_PHASE(S);
    }
    if (!D.layer_norm) { mlp_fwd(N, 0, N.n_layers, theta, S, out_act); return; }
    const int H = N.L[0].n;
    linear_fwd(N.L[0], theta, S.xin, S.xp, S.h1, S.hp, ACT_RELU, S.rc);
    FRL_PHASE(S);
    ln_rows(S.h1, S.hp, H, S.rc, X.rstd, X.mask);
    FRL_PHASE(S);
    linear_fwd(N.L[1], theta, S.h1, S.hp, S.h2, S.hp, ACT_RELU, S.rc);
    FRL_PHASE(S);
    ln_rows(S.h2, S.hp, H, S.rc, X.rstd + S.rc, X.mask + S.rc * kMappoMaskWords);
    FRL_PHASE(S);
    linear_fwd(N.L[2], theta, S.h2, S.hp, S.outb, S.op, out_act, S.rc);
    FRL_PHASE(S);
}

// Backward of the same: head delta in outb (zero in padded columns and invalid rows), gradients to G as `gs` says.  Ends with a barrier.
__device__ __forceinline__ void mappo_bwd(const EngineDesc& D, const NetDesc& N, g_cf theta, g_f G, const Lds& S, const MappoLds& X, int gs) {
    if (!D.layer_norm) { mlp_bwd(N, 0, N.n_layers, theta, G, S, gs, false, 0, 0); return; }
    const int H = N.L[0].n;
    linear_bwd_dw(N.L[2], G, S.outb, S.op, S.h2, S.hp, S.rc, gs);
    linear_bwd_dx(N.L[2], theta, S.outb, S.op, X.dbuf, S.hp, ACT_NONE, S.rc, 0, N.L[2].k_pad / 16);
    FRL_PHASE(S);
    ln_bwd_rows(X.dbuf, S.h2, S.hp, H, S.rc, X.rstd + S.rc, X.mask + S.rc * kMappoMaskWords);
    FRL_PHASE(S);
    linear_bwd_dw(N.L[1], G, X.dbuf, S.hp, S.h1, S.hp, S.rc, gs);
    linear_bwd_dx(N.L[1], theta, X.dbuf, S.hp, S.h2, S.hp, ACT_NONE, S.rc, 0, N.L[1].k_pad / 16);      // (h2's xhat is spent)
    FRL_PHASE(S);
    ln_bwd_rows(S.h2, S.h1, S.hp, H, S.rc, X.rstd, X.mask);
    FRL_PHASE(S);
    linear_bwd_dw(N.L[0], G, S.h2, S.hp, S.xin, S.xp, S.rc, gs);
    FRL_PHASE(S);
}

// ---- per-row head arithmetic.  `adv` / `vt` point at the learner's [T][n_agents] matrices, row t's columns [c0, c1) take part:
// one column (the agent's own) on IPPO engines, all of them on MAPPO engines (MAPPO.py:410-412: ratios [m, 1] x adv[index] [m, n]).

// the clipped surrogate of one row (onpolicy.hpp's surrogate_term per column): adds sum_j -min(ratio A_j, clamp(ratio) A_j) to `loss`,
// returns d (that sum) / d (sum of log-probs).  The critic's side of the same columns is onpolicy.hpp's value_row.
__device__ __forceinline__ float surrogate_row(float ratio, g_cf adv_row, int c0, int c1, float clip, float& loss) {
    float open = 0.f;
    for (int j = c0; j < c1; ++j) open += surrogate_term(ratio, adv_row[j], clip, loss);
    return -open * ratio;
}

// the critic's input of agent i: its own observation block, or all blocks (they are contiguous in a record, in agent order)
struct CriticIn { int obs, nobs, width; };
__device__ __forceinline__ CriticIn critic_in(const EngineDesc& D, int i) {
    const RecordDesc& R = D.rec;
    if (mappo_joint(D.algo)) return CriticIn{R.obs_off[0], R.nobs_off[0], R.obs_total};
    return CriticIn{R.obs_off[i], R.nobs_off[i], R.obs_dim[i]};
}

// the state segment of a critic's chunk (MAPPO_for_mask_action_state.py: kernels_mappo_state.hip): columns [dst0, dst0 + sd) of the nv
// valid rows = the state block (record columns [src0, src0 + sd)) of ring rows row0 .. row0 + nv - 1, zeros in the rows behind them.  A
// straight copy: consecutive threads read consecutive floats of a record, no index load
__device__ __forceinline__ void state_cols(lds_f X, int ldx, int rc, int nv, int row0, g_cf ring, int stride, int src0, int sd, int dst0) {
    for (int e = threadIdx.x; e < rc * sd; e += kWG) {
        const int r = e / sd, c = e - r * sd;
        X[r * ldx + dst0 + c] = r < nv ? ring[(size_t)(row0 + r) * stride + src0 + c] : 0.f;
    }
}

// ---- all K_epochs x minibatch steps of one net of (learner p, agent i) by the calling workgroup: the actor (net 2i) or the critic
// (net 2i+1), each step with its own Adam.  kWeighted (HAPPO.py:415): a row's surrogate and its gradient are multiplied by factor[t]
// (nullptr: 1, not read); the entropy term is not weighted.  Without it this is MAPPO.py:399-436 / IPPO.py:281-316 as they stand.
// kMasked (MAPPO_for_mask_action.py:349-352): the discrete actor's row is CategoricalMasked under the mask block of its ring record
// (D.mask_off: frl_action_mask_set); the critic's steps and the continuous actor's are untouched.
// kState (MAPPO_for_mask_action_state.py:371-373): the critic's row is [obs blocks of ring row idx[r] | state block], the state block
// that of ring row s + r (D.state_rows 0: the reference's `state` is not indexed) or of row idx[r] (1); the actor's steps are untouched.
template <bool kWeighted, bool kMasked = false, bool kState = false>
__device__ __forceinline__ void mappo_steps(const EngineDesc& D, const MappoArgs& a, const Lds& S, const MappoLds& X, int p, int i, bool do_actor,
                                            g_cf factor) {
    const int n = D.n_agents, u = p * n + i;
    const int T = a.horizon, mb = a.minibatch, rc = D.rc;
    const int net = 2 * i + (do_actor ? 0 : 1);
    const NetDesc& N = D.net[net];
    const RecordDesc& R = D.rec;
    const size_t off = (size_t)p * D.learner_stride + D.net_off[net];
    g_f th = as_global(D.theta + off);
    g_f G = as_global(D.grad + off);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_cf adv = as_global(a.adv + (size_t)p * T * n);
    g_cf vt = as_global(a.vtarget + (size_t)p * T * n);
    const bool discrete = D.n_discrete > 0;
    const int c0 = mappo_joint(D.algo) ? 0 : i, c1 = mappo_joint(D.algo) ? n : i + 1;      // advantage / target columns of a row
    const int O = R.obs_dim[i], A = D.net[2 * i].L[2].n;
    const int logp_col = R.extra_off + (R.act_off[i] - R.act_off[0]);                       // the log-prob blocks come first, in agent order
    const CriticIn ci = critic_in(D, i);
    const int npad = N.L[2].n_pad;
    int mask_col = 0;                                                                       // agent i's mask block: behind the earlier agents'
    if constexpr (kMasked) {
        mask_col = D.mask_off;
        for (int j = 0; j < i; ++j) mask_col += D.net[2 * j].L[2].n;
    }
    int* steps = D.steps + (size_t)p * (kMaxNets + 1);
    int t_adam = steps[net];
    const int n_mb = (T + mb - 1) / mb;
    float* trace = a.trace + (size_t)u * a.k_epochs * n_mb * 2;
    LearnArgs la = {};
    la.huber = a.huber;
    la.huber_delta = a.huber_delta;
    float last = 0.f;
    // a row's surrogate: into `lossp` and as d / d (sum of log-probs), weighted by the row's factor where the kernel has one
    auto surrogate = [&](float ratio, int t, float invmn, float& lossp) {
        if constexpr (kWeighted) {
            const float f = factor ? factor[t] : 1.f;
            float row = 0.f;
            const float g = surrogate_row(ratio, adv + (size_t)t * n, c0, c1, a.clip, row);
            lossp += f * row;
            return f * g * invmn;
        } else {
            return surrogate_row(ratio, adv + (size_t)t * n, c0, c1, a.clip, lossp) * invmn;
        }
    };

    for (int k = 0; k < a.k_epochs; ++k) {
        g_ci perm = as_global_i(a.perm + ((size_t)u * a.k_epochs + k) * T);
        for (int s = 0; s < T; s += mb) {
            const int m = min(mb, T - s);
            const float invm = 1.f / (float)m, invmn = 1.f / (float)(m * (c1 - c0));
            g_ci idx = perm + s;
            const int j_tr = k * n_mb + s / mb;
            float loss = 0.f;
            if (do_actor) {
                // ---------------- clipped surrogate - entropy_coefficient * mean entropy (MAPPO.py:399-412, IPPO.py:281-294)
                float lossp = 0.f, entp = 0.f, gls = 0.f, ent = 0.f;
                if (!discrete && threadIdx.x < A) ent = kHalfLog2PiPlusHalf + clamp_range(th[N.extra_off + threadIdx.x], kLogStdMin, kLogStdMax);
                const float ent_sum = block_sum(ent, S.red);          // Normal's entropy: the same for every row
                for (int r0 = 0; r0 < m; r0 += rc) {
                    const int nv = min(rc, m - r0);
                    gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, R.obs_off[i], O, 0);
                    zero_cols(S.xin, S.xp, rc, O, N.L[0].k_pad);
                    __syncthreads();
                    mappo_fwd(D, N, th, S, X, O, discrete ? ACT_NONE : ACT_TANH);          // mean = tanh(mean_layer(.))
                    if (discrete) {
                        // Categorical, or CategoricalMasked under the row's mask block: onpolicy.hpp's one-thread-per-row head
                        cat_head_delta(S, nv, A, npad, a.ent_coef * invm,
                            [&](int r, lds_cf z) {
                                if constexpr (kMasked) return masked_cat_row(z, ring + (size_t)idx[r0 + r] * R.stride + mask_col, A);
                                else return cat_row(z, A);
                            },
                            [&](int r) { return (int)ring[(size_t)idx[r0 + r] * R.stride + R.act_off[i]]; },
                            [&](int r, float lp_now, float entr) {
                                const int t = idx[r0 + r];
                                const float coef = surrogate(expf(lp_now - ring[(size_t)t * R.stride + logp_col]), t, invmn, lossp);
                                entp += entr;
                                return coef;
                            });
                    } else {
                        if (threadIdx.x < rc) {
                            const int r = threadIdx.x;
                            float coef = 0.f;
                            if (r < nv) {
                                const int t = idx[r0 + r];
                                g_cf rec = ring + (size_t)t * R.stride;
                                const float lp_now = normal_row_logp(rec + R.act_off[i], S.outb + r * S.op, th + N.extra_off, A, kLogStdMin, kLogStdMax);
                                float lp_old = 0.f;
                                for (int c = 0; c < A; ++c) lp_old += rec[logp_col + c];
                                coef = surrogate(expf(lp_now - lp_old), t, invmn, lossp);
                            }
                            S.dabuf[r * S.ap] = coef;      // d loss / d sum_c logp_now
                        }
                        normal_head_delta(S, nv, A, npad, idx + r0, ring, R.stride, R.act_off[i], th + N.extra_off, kLogStdMin, kLogStdMax, gls);
                    }
                    mappo_bwd(D, N, th, G, S, X, r0 == 0 ? GS_STORE : GS_ADD);
                }
                if (!discrete && threadIdx.x < A)
                    G[N.extra_off + threadIdx.x] = log_std_grad_open(th[N.extra_off + threadIdx.x], kLogStdMin, kLogStdMax) ? (gls - a.ent_coef) : 0.f;
                const float surr = block_sum(lossp, S.red) * invmn;
                const float entm = discrete ? block_sum(entp, S.red) * invm : ent_sum;
                loss = surr - a.ent_coef * entm;
            } else {
                // ---------------- critic: the loss of v_target[idx] against V (MAPPO.py:416-436, IPPO.py:300-316)
                float lossp = 0.f;
                for (int r0 = 0; r0 < m; r0 += rc) {
                    const int nv = min(rc, m - r0);
                    gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, ci.obs, ci.width, 0);
                    if constexpr (kState) {
                        if (D.state_rows) gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, D.state_off, D.state_dim, ci.width);
                        else state_cols(S.xin, S.xp, rc, nv, s + r0, ring, R.stride, D.state_off, D.state_dim, ci.width);
                        zero_cols(S.xin, S.xp, rc, ci.width + D.state_dim, N.L[0].k_pad);
                    } else {
                        zero_cols(S.xin, S.xp, rc, ci.width, N.L[0].k_pad);
                    }
                    __syncthreads();
                    mappo_fwd(D, N, th, S, X, kState ? ci.width + D.state_dim : ci.width, ACT_NONE);
                    if (threadIdx.x < rc) {
                        const int r = threadIdx.x;
                        float d = 0.f;
                        if (r < nv) d = value_row(la, S.outb[r * S.op], vt + (size_t)idx[r0 + r] * n, c0, c1, lossp) * invmn;
                        S.outb[r * S.op] = d;
                        for (int c = 1; c < npad; ++c) S.outb[r * S.op + c] = 0.f;
                    }
                    __syncthreads();
                    mappo_bwd(D, N, th, G, S, X, r0 == 0 ? GS_STORE : GS_ADD);
                }
                loss = block_sum(lossp, S.red) * invmn;
            }
            __syncthreads();
            ++t_adam;
            adam_net(N.size, th, as_global(D.m + off), as_global(D.v + off), G, nullptr, do_actor ? a.actor_lr : a.critic_lr, a.adam_eps, a.beta1,
                     a.beta2, 0.f, a.clip_norm, t_adam, 0.f, S.red);
            __syncthreads();
            if (threadIdx.x == 0) trace[2 * j_tr + (do_actor ? 0 : 1)] = loss;
            last = loss;
        }
    }
    if (threadIdx.x == 0) {
        float* st = D.stats + (size_t)u * ST_COUNT;
        steps[net] = t_adam;
        st[do_actor ? ST_ACTOR_LOSS : ST_CRITIC_LOSS] = last;
    }
}

}  // namespace frl
