// PPO on-policy update: value pass -> wave-scan GAE (+ advantage normalisation) -> ONE persistent
// launch running all K_epochs x (horizon / minibatch) clipped-surrogate actor and MSE critic
// steps of a learner (PPO_file/PPO_with_tricks.py:290-354).  The reference does the GAE
// recurrence as a sequential host loop (:308-311) after a device->host copy and launches a few
// hundred tiny kernels per minibatch; here the rollout never leaves HBM.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/onpolicy.hpp"
#include "device/gae.hpp"
#include "device/special.hpp"
#include "device/ppo_timing.hpp"

namespace frl {


// ---- td_delta = r + gamma*(1-done)*V(s') - V(s) for every stored row (PPO_with_tricks.py:304-306)
__global__ __launch_bounds__(256) void ppo_values_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc, rc = D.rc, T = a.horizon;
    const int nv = min(rc, T - r0);
    const NetDesc& N = D.net[1];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    g_cf theta = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[1]);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    const int O = R.obs_dim[0], kpad = N.L[0].k_pad;
    float v0 = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        const int src = pass == 0 ? R.obs_off[0] : R.nobs_off[0];
        load_rows(S.xin, S.xp, rc, nv, ring, r0, R.stride, src, O, kpad);
        if (D.obs_norm_on) {
            __syncthreads();
            normalize_cols(S.xin, S.xp, nv, 0, O, as_global(D.obsnorm + (size_t)p * (1 + 3 * O)), O);
        }
        __syncthreads();
        mlp_fwd(N, 0, N.n_layers, theta, S, ACT_NONE);
        if (threadIdx.x < nv) {
            const float v = S.outb[threadIdx.x * S.op];
            if (pass == 0) {
                v0 = v;
            } else {
                g_cf rec = ring + (size_t)(r0 + threadIdx.x) * R.stride;
                const size_t o = (size_t)p * T + r0 + threadIdx.x;
                a.vs[o] = v0;
                a.td[o] = rec[R.rew_off] + a.gamma * (1.f - rec[R.done_off]) * v - v0;
            }
        }
        __syncthreads();
    }
}

// ---- GAE: the affine suffix scan gae_scan (device/gae.hpp), v_target and the optional advantage normalisation
__global__ __launch_bounds__(256) void ppo_gae_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a) {
    __shared__ float lds_s[16];
    lds_f lds = (lds_f)lds_s;
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x, T = a.horizon;
    const RecordDesc& R = D.rec;
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_f adv_raw = as_global(a.adv_raw + (size_t)p * T);
    g_f adv = as_global(a.adv + (size_t)p * T);
    g_cf vs = as_global(a.vs + (size_t)p * T);
    g_f vt = as_global(a.vtarget + (size_t)p * T);
    const int adv_done_col = R.extra_off + R.extra - 1;   // last extra column (PPO_file/Buffer.py:282)
    gae_scan(as_global(a.td + (size_t)p * T), ring, R.stride, adv_done_col, T, a.gamma * a.lmbda, adv_raw, lds);
    // v_target = adv + V(s) (:313); optional (adv - mean)/(std + 1e-8), unbiased std (:314-315)
    float s1 = 0.f;
    for (int i = threadIdx.x; i < T; i += kWG) {
        const float x = adv_raw[i];
        vt[i] = x + vs[i];
        s1 += x;
    }
    if (!a.adv_norm) {
        for (int i = threadIdx.x; i < T; i += kWG) adv[i] = adv_raw[i];
        return;
    }
    normalize_adv(s1, T, adv_raw, adv, [](int i) { return i; }, lds + 8);
}

// ---- PPO_advance/Buffer.py:480-507 `compute_returns_and_advantage` (stable-baselines3's form): the values were stored
// at rollout time; float64 throughout (the reference scans float64 NumPy arrays with Python-float gamma / lambda), one
// cast to float32 at the end (PPO_2.py:223-224).  Same affine suffix scan as gae_scan, in double (gae.hpp's AffineD).
__global__ __launch_bounds__(256) void ppo_gae_sb3_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a) {
    __shared__ double lds_d[8];
    __shared__ float lds_s[16];
    lds_f lds = (lds_f)lds_s;
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x, T = a.horizon, t = threadIdx.x;
    const RecordDesc& R = D.rec;
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_f adv_raw = as_global(a.adv_raw + (size_t)p * T);
    g_f adv = as_global(a.adv + (size_t)p * T);
    g_f vt = as_global(a.vtarget + (size_t)p * T);
    const int ad_col = R.extra_off + R.extra - 1, v_col = ad_col - 1;
    const double gam = a.gamma_d, c = a.gamma_d * a.lmbda_d, last = (double)a.last_value[p];
    auto step = [&](int i, double& g, double& delta) {
        g_cf rec = ring + (size_t)i * R.stride;
        const double nv = (i == T - 1) ? last : (double)rec[R.stride + v_col];
        delta = (double)rec[R.rew_off] + gam * nv * (1.0 - (double)rec[R.done_off]) - (double)rec[v_col];
        g = c * (1.0 - (double)rec[ad_col]);
    };
    const int L = (T + kWG - 1) / kWG, s0 = min(t * L, T), s1 = min(s0 + L, T);
    AffineD f{1.0, 0.0};
    for (int i = s1 - 1; i >= s0; --i) {
        double g, d;
        step(i, g, d);
        f = AffineD{g * f.a, d + g * f.b};
    }
    const int lane = t & 63, w = t >> 6;
    AffineD s = f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        AffineD o{__shfl_down(s.a, off, 64), __shfl_down(s.b, off, 64)};
        if (lane + off < 64) s = compose(s, o);
    }
    if (lane == 0) { lds_d[2 * w] = s.a; lds_d[2 * w + 1] = s.b; }
    __syncthreads();
    double right = 0.0;
    for (int ww = kWaves - 1; ww > w; --ww) right = lds_d[2 * ww] * right + lds_d[2 * ww + 1];
    const double mine = s.a * right + s.b;
    double x = __shfl_down(mine, 1, 64);
    if (lane == 63) x = right;
    float s1f = 0.f;
    for (int i = s1 - 1; i >= s0; --i) {
        double g, d;
        step(i, g, d);
        x = d + g * x;
        const float xf = (float)x;
        adv_raw[i] = xf;
        vt[i] = (float)(x + (double)ring[(size_t)i * R.stride + v_col]);
        s1f += xf;
    }
    __syncthreads();
    if (!a.adv_norm) {
        for (int i = t; i < T; i += kWG) adv[i] = adv_raw[i];
        return;
    }
    normalize_adv(s1f, T, adv_raw, adv, [](int i) { return i; }, lds + 8);
}

// ---- np.random.permutation(horizon) per (learner, epoch) (PPO_with_tricks.py:320) on the device when the caller does not
// supply the draws: sort (32 random bits, index) pairs — a bitonic sort of one 64-bit word per row in LDS.  (On the host
// this was 13 of the 65 ms of a 256-learner learn(): a Fisher-Yates of P*K*T swaps plus a 21 MB upload.)
__global__ __launch_bounds__(256) void ppo_perm_kernel(int* __restrict__ perm, int T, int Tpad, unsigned long long counter,
                                                        unsigned long long seed) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    const int k = blockIdx.x, p = blockIdx.y, K = gridDim.x;
    const unsigned long long key = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(p + 1);
    for (int i = threadIdx.x; i < Tpad; i += kWG) {
        unsigned long long v = ~0ull;                                   // padding sorts to the end
        if (i < T) {
            const Philox4 r = philox4x32_10(counter, 0x7000u + (unsigned)k, (unsigned)(i >> 2), key);
            const unsigned w = (i & 3) == 0 ? r.x : ((i & 3) == 1 ? r.y : ((i & 3) == 2 ? r.z : r.w));
            v = ((unsigned long long)w << 32) | (unsigned)i;
        }
        keys[i] = v;
    }
    __syncthreads();
    for (int size = 2; size <= Tpad; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < Tpad / 2; t += kWG) {
                const int lo = 2 * t - (t & (stride - 1));              // element whose partner is lo + stride
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    int* out = perm + ((size_t)p * K + k) * T;
    for (int i = threadIdx.x; i < T; i += kWG) out[i] = (int)(keys[i] & 0xFFFFFFFFu);
}

// stand-alone K3 entry (frl_gae): adv_done given as a dense array
__global__ __launch_bounds__(256) void gae_dense_kernel(const float* __restrict__ delta, const float* __restrict__ adv_done,
                                                         int T, float c, float* __restrict__ adv) {
    __shared__ float lds_s[16];
    const size_t o = (size_t)blockIdx.x * T;
    gae_scan(as_global(delta + o), as_global(adv_done + o), 1, 0, T, c, as_global(adv + o), (lds_f)lds_s);
}

// ---- all minibatch updates of one learner in one launch
__global__ __launch_bounds__(256) void ppo_update_kernel(const EngineDesc* __restrict__ Dp, PpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    // blockIdx.y: 0 = the actor's steps, 1 = the critic's.  Within learn() the two nets never read each other (the
    // advantages and value targets were fixed by the GAE pass, PPO_with_tricks.py:300-316), so their K_epochs x minibatch
    // step sequences run as two independent persistent workgroups.
    const int p = blockIdx.x, T = a.horizon, mb = a.minibatch, rc = D.rc;
    const bool do_actor = (blockIdx.y == 0), do_critic = (blockIdx.y == 1);
    const NetDesc& NA = D.net[0];
    const NetDesc& NC = D.net[1];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const size_t offA = (size_t)p * D.learner_stride + D.net_off[0], offC = (size_t)p * D.learner_stride + D.net_off[1];
    g_f thA = as_global(D.theta + offA);
    g_f thC = as_global(D.theta + offC);
    g_f gA = as_global(D.grad + offA);
    g_f gC = as_global(D.grad + offC);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_cf adv = as_global(a.adv + (size_t)p * T);
    g_cf vt = as_global(a.vtarget + (size_t)p * T);
    const bool discrete = D.n_discrete > 0, beta = D.beta_actor != 0;
    g_cf bn = D.obs_norm_on ? as_global(D.obsnorm + (size_t)p * (1 + 3 * R.obs_dim[0])) : nullptr;
    const int O = R.obs_dim[0], A = discrete ? D.n_discrete : R.act_dim[0], logp_col = R.extra_off;
    const int napad = NA.L[NA.n_layers - 1].n_pad, ncpad = NC.L[NC.n_layers - 1].n_pad;
    int* steps = D.steps + (size_t)p * (kMaxNets + 1);
    int tA = steps[0], tC = steps[1];
    const int n_mb = (T + mb - 1) / mb;
    float* trace = a.trace + (size_t)p * a.k_epochs * n_mb * 2;
    PPO_T0();

    for (int k = 0; k < a.k_epochs; ++k) {
        g_ci perm = as_global_i(a.perm + ((size_t)p * a.k_epochs + k) * T);
        for (int s = 0; s < T; s += mb) {
            const int m = min(mb, T - s);
            const float invm = 1.f / (float)m;
            g_ci idx = perm + s;
            const int j_tr = k * n_mb + s / mb;
            if (do_actor) {
            // ---------------- actor: clipped surrogate + entropy bonus (:324-346)
            float lossp = 0.f, gls = 0.f, ent = 0.f;
            if (!discrete && !beta && threadIdx.x < A) {
                ent = kHalfLog2PiPlusHalf + clamp_range(thA[NA.extra_off + threadIdx.x], kLogStdMin, kLogStdMax);
            }
            const float ent_sum = block_sum(ent, S.red);          // same for every row
            for (int r0 = 0; r0 < m; r0 += rc) {
                const int nv = min(rc, m - r0);
                gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, R.obs_off[0], O, 0);
                zero_cols(S.xin, S.xp, rc, O, NA.L[0].k_pad);
                if (bn) { __syncthreads(); normalize_cols(S.xin, S.xp, nv, 0, O, bn, O); }
                __syncthreads();
                PPO_T(0);
                mlp_fwd(NA, 0, NA.n_layers, thA, S, (discrete || beta) ? ACT_NONE : ACT_TANH);    // mean = tanh(mean_layer(.)) (:99)
                PPO_T(1);
                if (beta) {
                    // Beta(alpha, beta) per action dimension (:325-332): alpha = softplus(z_a) + 1, beta = softplus(z_b) + 1;
                    // log_prob(a) = (alpha-1) ln a + (beta-1) ln(1-a) - ln B; entropy = ln B - (alpha-1) psi(alpha) -
                    // (beta-1) psi(beta) + (alpha+beta-2) psi(alpha+beta), summed over dimensions.  One thread per row.
                    if (threadIdx.x < rc) {
                        const int r = threadIdx.x;
                        if (r < nv) {
                            g_cf rec = ring + (size_t)idx[r0 + r] * R.stride;
                            double lp_now = 0.0, lp_old = 0.0, entr = 0.0;
                            for (int c = 0; c < A; ++c) {
                                const float za = S.outb[r * S.op + c], zb = S.outb[r * S.op + A + c];
                                const double al = (double)(za > 20.f ? za : log1pf(expf(za))) + 1.0;
                                const double be = (double)(zb > 20.f ? zb : log1pf(expf(zb))) + 1.0;
                                const double x = (double)rec[R.act_off[0] + c];
                                const double lB = lbeta_d(al, be);
                                lp_now += (al - 1.0) * log(x) + (be - 1.0) * log1p(-x) - lB;
                                lp_old += (double)rec[logp_col + c];
                                entr += lB - (al - 1.0) * digamma_d(al) - (be - 1.0) * digamma_d(be) + (al + be - 2.0) * digamma_d(al + be);
                            }
                            const float ratio = expf((float)(lp_now - lp_old));
                            float surr = 0.f;
                            const float open = surrogate_term(ratio, adv[idx[r0 + r]], a.clip, surr);
                            lossp += surr - a.ent_coef * (float)entr;
                            const double coef = (double)(open * (-invm) * ratio), ce = (double)(a.ent_coef * invm);
                            for (int c = 0; c < A; ++c) {
                                const float za = S.outb[r * S.op + c], zb = S.outb[r * S.op + A + c];
                                const double al = (double)(za > 20.f ? za : log1pf(expf(za))) + 1.0;
                                const double be = (double)(zb > 20.f ? zb : log1pf(expf(zb))) + 1.0;
                                const double x = (double)rec[R.act_off[0] + c];
                                const double psi_ab = digamma_d(al + be), tri_ab = trigamma_d(al + be);
                                const double dlp_a = log(x) - digamma_d(al) + psi_ab, dlp_b = log1p(-x) - digamma_d(be) + psi_ab;
                                const double dH_a = -(al - 1.0) * trigamma_d(al) + (al + be - 2.0) * tri_ab;
                                const double dH_b = -(be - 1.0) * trigamma_d(be) + (al + be - 2.0) * tri_ab;
                                const double sa = za > 20.f ? 1.0 : 1.0 / (1.0 + exp(-(double)za));     // d softplus / dz
                                const double sb = zb > 20.f ? 1.0 : 1.0 / (1.0 + exp(-(double)zb));
                                S.abuf[r * S.ap + c] = (float)((coef * dlp_a - ce * dH_a) * sa);
                                S.abuf[r * S.ap + A + c] = (float)((coef * dlp_b - ce * dH_b) * sb);
                            }
                            for (int c = 2 * A; c < napad; ++c) S.abuf[r * S.ap + c] = 0.f;
                        } else {
                            for (int c = 0; c < napad; ++c) S.abuf[r * S.ap + c] = 0.f;
                        }
                        for (int c = 0; c < napad; ++c) S.outb[r * S.op + c] = S.abuf[r * S.ap + c];
                    }
                    __syncthreads();
                } else if (discrete) {
                    // Categorical(probs = softmax(l3)) (:333-336), or Categorical(logits = l3) on a cat_logits engine: the softmax,
                    // log-prob of the stored action, entropy, ratio and the logits' delta are onpolicy.hpp's one-thread-per-row head
                    cat_head_delta(S, nv, A, napad, a.ent_coef * invm,
                        [&](int, lds_cf z) { return cat_row(z, A, D.cat_logits ? CAT_LOGITS_Q : CAT_PROBS); },
                        [&](int r) { return (int)ring[(size_t)idx[r0 + r] * R.stride + R.act_off[0]]; },
                        [&](int r, float lp_now, float entr) {
                            const float ratio = expf(lp_now - ring[(size_t)idx[r0 + r] * R.stride + logp_col]);
                            float surr = 0.f;
                            const float open = surrogate_term(ratio, adv[idx[r0 + r]], a.clip, surr);
                            lossp += surr - a.ent_coef * entr;
                            return open * (-invm) * ratio;
                        });
                } else {
                // per-row ratio and d loss / d sum(logp)
                if (threadIdx.x < rc) {
                    const int r = threadIdx.x;
                    float coef = 0.f;
                    if (r < nv) {
                        g_cf rec = ring + (size_t)idx[r0 + r] * R.stride;
                        const float lp_now = normal_row_logp(rec + R.act_off[0], S.outb + r * S.op, thA + NA.extra_off, A, kLogStdMin, kLogStdMax);
                        float lp_old = 0.f;
                        for (int c = 0; c < A; ++c) lp_old += rec[logp_col + c];
                        const float ratio = expf(lp_now - lp_old);
                        coef = surrogate_term(ratio, adv[idx[r0 + r]], a.clip, lossp) * (-invm) * ratio;   // d loss / d sum_c logp_now
                    }
                    S.dabuf[r * S.ap] = coef;
                }
                normal_head_delta(S, nv, A, napad, idx + r0, ring, R.stride, R.act_off[0], thA + NA.extra_off, kLogStdMin, kLogStdMax, gls);
                }
                // one call site for the three policy distributions (every inlined copy of the backward pass is ~20 k
                // instructions of a kernel that walks its whole code once per minibatch step)
                PPO_T(2);
                mlp_bwd(NA, 0, NA.n_layers, thA, gA, S, r0 == 0 ? GS_STORE : GS_ADD, false, 0, 0);
                PPO_T(3);
            }
            if (!discrete && !beta && threadIdx.x < A) {
                const float raw = thA[NA.extra_off + threadIdx.x];
                gA[NA.extra_off + threadIdx.x] = log_std_grad_open(raw, kLogStdMin, kLogStdMax) ? (gls - a.ent_coef) : 0.f;
            }
            const float aloss = block_sum(lossp, S.red) * invm - ((discrete || beta) ? 0.f : a.ent_coef * ent_sum);
            __syncthreads();
            ++tA;
            if (a.optimizer == 1)
                cadamw_net(NA, thA, as_global(D.m + offA), as_global(D.v + offA), gA, a.actor_lr, a.adam_eps, a.beta1, a.beta2, a.clip_norm, tA, S.red);
            else
                adam_net(NA.size, thA, as_global(D.m + offA), as_global(D.v + offA), gA, nullptr, a.actor_lr, a.adam_eps, a.beta1, a.beta2, 0.f,
                         a.clip_norm, tA, 0.f, S.red);
            __syncthreads();
            PPO_T(4);
            if (threadIdx.x == 0) trace[2 * j_tr] = aloss;
            }
            if (!do_critic) continue;
            // ---------------- critic: mse(v_target[idx], V(obs[idx])) (:349-351)
            float closs_p = 0.f;
            for (int r0 = 0; r0 < m; r0 += rc) {
                const int nv = min(rc, m - r0);
                gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, R.obs_off[0], O, 0);
                zero_cols(S.xin, S.xp, rc, O, NC.L[0].k_pad);
                if (bn) { __syncthreads(); normalize_cols(S.xin, S.xp, nv, 0, O, bn, O); }
                __syncthreads();
                PPO_T(0);
                mlp_fwd(NC, 0, NC.n_layers, thC, S, ACT_NONE);
                PPO_T(1);
                critic_delta_rows(S, nv, ncpad, idx + r0, vt, 1.f, invm, closs_p);
                PPO_T(2);
                mlp_bwd(NC, 0, NC.n_layers, thC, gC, S, r0 == 0 ? GS_STORE : GS_ADD, false, 0, 0);
                PPO_T(3);
            }
            const float closs = block_sum(closs_p, S.red) * invm;
            __syncthreads();
            ++tC;
            if (a.optimizer == 1)      // one AdamW over both nets: the actor's learning rate (PPO.py:121)
                cadamw_net(NC, thC, as_global(D.m + offC), as_global(D.v + offC), gC, a.actor_lr, a.adam_eps, a.beta1, a.beta2, a.clip_norm, tC, S.red);
            else
                adam_net(NC.size, thC, as_global(D.m + offC), as_global(D.v + offC), gC, nullptr, a.critic_lr, a.adam_eps, a.beta1, a.beta2, 0.f,
                         a.clip_norm, tC, 0.f, S.red);
            __syncthreads();
            PPO_T(4);
            if (threadIdx.x == 0) trace[2 * j_tr + 1] = closs;
        }
    }
    if (threadIdx.x == 0) {
        float* st = D.stats + (size_t)p * D.n_agents * ST_COUNT;
        const int j = a.k_epochs * n_mb - 1;
        if (do_actor) { steps[0] = tA; st[ST_ACTOR_LOSS] = trace[2 * j]; }
        if (do_critic) { steps[1] = tC; st[ST_CRITIC_LOSS] = trace[2 * j + 1]; }
    }
    PPO_TDUMP();
}

}  // namespace frl
