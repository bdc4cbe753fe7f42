// GAIL's policy side (GAIL_file/PPO2.py:235-307, `PPO.PPO_learn`) on an ALGO_GAIL_PPO engine: net 0 the actor, net 1 the critic, both
// obs -> H -> H -> out with LeakyReLU (GAIL's config) or ReLU (PPO2's own) hidden layers.  Launch chain (frl_api_gail_ppo.inc):
//     gail_ppo_prepare_kernel -> gail_ppo_gae_kernel -> [ppo_perm_kernel] -> gail_ppo_update_kernel
// What differs from kernels_ppo.hip, and why this is a unit of its own: the old log-prob is not stored at rollout time but recomputed
// over the whole horizon with the pre-update actor; the TD residual bootstraps from the NEXT ROW's V(s) even across an episode end
// (mask_1 == 1, :254) and from the caller's last_value behind the last row — next_obs is never read; log_std is clamped to the ENGINE's
// range (EngineDesc::log_std_min / _max) with torch.clamp's closed-bound gradient gate; the critic loss carries value_loss_coef; the
// discrete policy is Categorical(logits=); both nets count the steps of the reference's single Adam.
// gail_ppo_act_kernel: the forward for frl_act on such an engine (LeakyReLU hidden layers, the engine's log_std range).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/act_common.hpp"
#include "device/gae.hpp"
#include "device/onpolicy.hpp"

namespace frl {

namespace {

// the forward of a 3-layer net whose hidden activation may be ACT_LEAKY_RELU; ends with a barrier
__device__ __forceinline__ void fwd3(const NetDesc& N, g_cf theta, const Lds& S, int out_act) {
    mlp_fwd_rows(N, 0, N.n_layers, theta, S, out_act, NoRowConsumer{}, NoRowConsumer{}, std::true_type{});
}

// log pi(a | s) of chunk row r from the actor's head row in outb: Normal(tanh mean, exp(clamp(log_std))) summed over dimensions
// (PPO2.py:250,282), or the log-softmax entry of the stored index (Categorical(logits=), :247,279)
__device__ __forceinline__ float row_logp(const EngineDesc& D, const NetDesc& NA, g_cf thA, const Lds& S, int r, g_cf rec, bool discrete, int A) {
    const RecordDesc& R = D.rec;
    if (discrete) {
        lds_cf z = S.outb + r * S.op;
        return cat_row(z, A, CAT_LOGITS_E).logit(z[min(max((int)rec[R.act_off[0]], 0), A - 1)]);
    }
    return normal_row_logp(rec + R.act_off[0], S.outb + r * S.op, thA + NA.extra_off, A, D.log_std_min, D.log_std_max);
}

}  // namespace

// ---- V(s_t) and log pi_old(a_t | s_t) for ring rows 0 .. T-1: one row load feeds both forwards.  grid = (row chunks, learners)
__global__ __launch_bounds__(256) void gail_ppo_prepare_kernel(const EngineDesc* __restrict__ Dp, GailPpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, rc = D.rc, r0 = blockIdx.x * rc, T = a.horizon;
    const int nv = min(rc, T - r0);
    const NetDesc& NA = D.net[0];
    const NetDesc& NC = D.net[1];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    g_cf thA = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[0]);
    g_cf thC = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[1]);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    const bool discrete = D.n_discrete > 0;
    const int O = R.obs_dim[0], kpad = NA.L[0].k_pad, A = discrete ? D.n_discrete : R.act_dim[0];      // (both first layers: the same k_pad)
    load_rows(S.xin, S.xp, rc, nv, ring, r0, R.stride, R.obs_off[0], O, kpad);
    __syncthreads();
    fwd3(NC, thC, S, ACT_NONE);
    const size_t o = (size_t)p * T + r0 + threadIdx.x;
    if ((int)threadIdx.x < nv) a.vs[o] = S.outb[threadIdx.x * S.op];
    __syncthreads();
    fwd3(NA, thA, S, discrete ? ACT_NONE : ACT_TANH);
    if ((int)threadIdx.x < nv)
        a.logp_old[o] = row_logp(D, NA, thA, S, threadIdx.x, ring + (size_t)(r0 + threadIdx.x) * R.stride, discrete, A);
}

// ---- PPO2.GAE (:186-233) with masks_1 == 1: td_t = r_t + gamma V(s_{t+1}) - V(s_t), V(s_T) = last_value — NO (1 - done) on the
// bootstrap; A_t = td_t + c (1 - done_t) A_{t+1}; returns = A + V; A <- (A - mean) / (unbiased std + 1e-8).  One workgroup per learner.
__global__ __launch_bounds__(256) void gail_ppo_gae_kernel(const EngineDesc* __restrict__ Dp, GailPpoArgs a) {
    __shared__ float lds_s[16];
    lds_f lds = (lds_f)lds_s;
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x, T = a.horizon;
    const RecordDesc& R = D.rec;
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_cf vs = as_global(a.vs + (size_t)p * T);
    g_f td = as_global(a.td + (size_t)p * T);
    g_f adv_raw = as_global(a.adv_raw + (size_t)p * T);
    g_f adv = as_global(a.adv + (size_t)p * T);
    g_f ret = as_global(a.returns + (size_t)p * T);
    const float last = a.last_value[p];
    for (int i = threadIdx.x; i < T; i += kWG) {
        const float r = a.rewards ? a.rewards[(size_t)p * T + i] : ring[(size_t)i * R.stride + R.rew_off];
        const float vn = (i == T - 1) ? last : vs[i + 1];
        td[i] = (r + a.gamma * vn) - vs[i];
    }
    __syncthreads();
    gae_scan(td, ring, R.stride, R.done_off, T, a.c, adv_raw, lds);
    float s1 = 0.f;
    for (int i = threadIdx.x; i < T; i += kWG) {
        const float x = adv_raw[i];
        ret[i] = x + vs[i];
        s1 += x;
    }
    normalize_adv(s1, T, adv_raw, adv, [](int i) { return i; }, lds + 8);
}

// ---- all K_epochs x ceil(T / mb) steps of one learner in one launch.  blockIdx.y: 0 = the actor's steps, 1 = the critic's: inside
// PPO_learn the two nets never read each other (advantages, returns and the old log-probs are fixed before the first step), and the
// reference's one Adam with two param groups steps each net with its own lr and the same count.
__global__ __launch_bounds__(256) void gail_ppo_update_kernel(const EngineDesc* __restrict__ Dp, GailPpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x, T = a.horizon, mb = a.minibatch, rc = D.rc;
    const bool do_actor = (blockIdx.y == 0);
    const NetDesc& N = D.net[do_actor ? 0 : 1];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const size_t off = (size_t)p * D.learner_stride + D.net_off[do_actor ? 0 : 1];
    g_f th = as_global(D.theta + off);
    g_f G = as_global(D.grad + off);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_cf adv = as_global(a.adv + (size_t)p * T);
    g_cf ret = as_global(a.returns + (size_t)p * T);
    g_cf lp_old = as_global(a.logp_old + (size_t)p * T);
    const bool discrete = D.n_discrete > 0;
    const int O = R.obs_dim[0], A = discrete ? D.n_discrete : R.act_dim[0];
    const int npad = N.L[N.n_layers - 1].n_pad;
    const float lo = D.log_std_min, hi = D.log_std_max;
    int* steps = D.steps + (size_t)p * (kMaxNets + 1);
    int t = steps[do_actor ? 0 : 1];
    const int n_mb = (T + mb - 1) / mb;
    float* trace = a.trace + (size_t)p * a.k_epochs * n_mb * 2;
    const int out_act = (do_actor && !discrete) ? ACT_TANH : ACT_NONE;

    for (int k = 0; k < a.k_epochs; ++k) {
        g_ci perm = as_global_i(a.perm + ((size_t)p * a.k_epochs + k) * T);
        for (int s = 0; s < T; s += mb) {
            const int m = min(mb, T - s);                         // (a short last minibatch: the mean over its own rows)
            const float invm = 1.f / (float)m;
            g_ci idx = perm + s;
            float lossp = 0.f, gls = 0.f, ent = 0.f;
            if (do_actor && !discrete && (int)threadIdx.x < A) ent = kHalfLog2PiPlusHalf + clamp_range(th[N.extra_off + threadIdx.x], lo, hi);
            const float ent_sum = block_sum(ent, S.red);          // the Normal's entropy does not depend on the row
            for (int r0 = 0; r0 < m; r0 += rc) {
                const int nv = min(rc, m - r0);
                gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, R.obs_off[0], O, 0);
                zero_cols(S.xin, S.xp, rc, O, N.L[0].k_pad);
                __syncthreads();
                fwd3(N, th, S, out_act);
                if (!do_actor) {
                    // ---------------- critic: value_loss_coef * mse(V(s[idx]), returns[idx]) (:295-298)
                    critic_delta_rows(S, nv, npad, idx + r0, ret, a.value_loss_coef, invm, lossp);
                } else if (discrete) {
                    // ---------------- Categorical(logits=) (:277-280): log-softmax, entropy -sum p log p, ratio, the logits' delta — onpolicy.hpp's
                    // one-thread-per-row head; the stored index is clamped to [0, A - 1] here and nowhere else
                    cat_head_delta(S, nv, A, npad, a.ent_weight * invm,
                        [&](int, lds_cf z) { return cat_row(z, A, CAT_LOGITS_E); },
                        [&](int r) { return min(max((int)ring[(size_t)idx[r0 + r] * R.stride + R.act_off[0]], 0), A - 1); },
                        [&](int r, float lp_now, float entr) {
                            const int row = idx[r0 + r];
                            const float ratio = expf(lp_now - lp_old[row]);
                            float surr = 0.f;
                            const float open = surrogate_term(ratio, adv[row], a.clip, surr);
                            lossp += surr - a.ent_weight * entr;
                            return open * (-invm) * ratio;
                        });
                } else {
                    // ---------------- Normal (:282-292): the row's ratio and d loss / d sum_c logp, then the head's and log_std's deltas
                    if ((int)threadIdx.x < rc) {
                        const int r = threadIdx.x;
                        float coef = 0.f;
                        if (r < nv) {
                            const int row = idx[r0 + r];
                            const float lp_now = row_logp(D, N, th, S, r, ring + (size_t)row * R.stride, false, A);
                            const float ratio = expf(lp_now - lp_old[row]);
                            coef = surrogate_term(ratio, adv[row], a.clip, lossp) * (-invm) * ratio;
                        }
                        S.dabuf[r * S.ap] = coef;
                    }
                    normal_head_delta(S, nv, A, npad, idx + r0, ring, R.stride, R.act_off[0], th + N.extra_off, lo, hi, gls);
                }
                // one call site for both nets and both distributions: every inlined copy of the backward pass is ~20 k instructions of a
                // kernel that walks its whole code once per minibatch step (kernels_ppo.hip)
                mlp_bwd(N, 0, N.n_layers, th, G, S, r0 == 0 ? GS_STORE : GS_ADD, false, 0, 0, std::true_type{});
            }
            if (do_actor && !discrete && (int)threadIdx.x < A) {
                // torch.clamp passes the gradient on the CLOSED range [lo, hi] (:38)
                const float raw = th[N.extra_off + threadIdx.x];
                G[N.extra_off + threadIdx.x] = log_std_grad_open(raw, lo, hi) ? (gls - a.ent_weight) : 0.f;
            }
            float loss = block_sum(lossp, S.red) * invm;
            if (do_actor) loss -= discrete ? 0.f : a.ent_weight * ent_sum;
            else loss *= a.value_loss_coef;
            __syncthreads();
            ++t;
            // clip_grad_norm_(net, 0.5) on this net alone, then its param group's Adam step (:303-307)
            adam_net(N.size, th, as_global(D.m + off), as_global(D.v + off), G, nullptr, do_actor ? a.p_lr : a.v_lr, 1e-8f, 0.9f, 0.999f, 0.f,
                     a.clip_norm, t, 0.f, S.red);
            __syncthreads();
            if (threadIdx.x == 0) trace[2 * (k * n_mb + s / mb) + (do_actor ? 0 : 1)] = loss;
        }
    }
    if (threadIdx.x == 0) {
        float* st = D.stats + (size_t)p * D.n_agents * ST_COUNT;
        const int j = a.k_epochs * n_mb - 1;
        steps[do_actor ? 0 : 1] = t;
        st[do_actor ? ST_ACTOR_LOSS : ST_CRITIC_LOSS] = trace[2 * j + (do_actor ? 0 : 1)];
    }
}

// ---- frl_act on an ALGO_GAIL_PPO engine: act_kernel's row load, the forward with the net's own hidden activation, then act_epilogue for
// the modes that read no log_std and the engine's clamp range for FRL_ACT_PPO_SAMPLE.  grid = (row chunks, learners)
__global__ __launch_bounds__(256) void gail_ppo_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, rc = D.rc, r0 = blockIdx.x * rc;
    const NetDesc& N = D.net[a.net];
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const int nv = min(rc, a.n_rows - r0);
    g_cf theta = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[a.net]);
    const int K = a.in_dim, kpad = N.L[0].k_pad, nout = N.L[N.n_layers - 1].n;
    g_cf in = as_global(a.in + ((size_t)p * a.n_rows + r0) * K);
    load_rows(S.xin, S.xp, rc, nv, in, 0, K, 0, K, kpad);
    __syncthreads();
    fwd3(N, theta, S, (a.mode == ACTM_TANH || a.mode == ACTM_PPO_SAMPLE) ? ACT_TANH : ACT_NONE);
    if (a.mode != ACTM_PPO_SAMPLE) {
        act_epilogue(D, a, N, theta, S.outb, S.op, nv, r0, p, nout);
        return;
    }
    // pi(s) (PPO2.py:94-101): Normal(mean, exp(clamp(log_std, lo, hi))).sample() = mean + std eps; the log-prob per dimension
    const unsigned long long key = D.seed + 0x9E3779B97F4A7C15ull * (p + 1);
    for (int e = threadIdx.x; e < nv * nout; e += kWG) {
        const int r = e / nout, c = e - r * nout;
        const size_t o = ((size_t)p * a.n_rows + r0 + r) * nout + c;
        const float mean = S.outb[r * S.op + c];
        const float ls = clamp_range(theta[N.extra_off + c], D.log_std_min, D.log_std_max), sd = expf(ls);
        float eps = 0.f;
        if (a.eps) eps = a.eps[o];
        else if (a.device_eps) {
            float n0, n1;
            normal2(philox4x32_10(a.rng_counter, 0x9200u, (unsigned)((r0 + r) * nout + c), key), n0, n1);
            eps = n0;
        }
        const float u = mean + sd * eps;
        if (a.out_logp) a.out_logp[o] = normal_logp(u - mean, sd, ls);
        a.out[o] = u;
    }
}

}  // namespace frl
