// MAPPO and IPPO (MAPPO_file/MAPPO.py:357-482, IPPO.py:252-322): per agent i an actor on its own observation (net 2i) and a critic
// (net 2i+1) on its own observation (IPPO) or on the concatenation of every agent's (MAPPO).  One learn() is
//     mappo_values_kernel -> gae_dense_kernel -> mappo_adv_kernel -> mappo_update_kernel
// and the update is ppo_update_kernel's shape: one persistent workgroup per (learner, agent, net) runs all K_epochs x minibatch steps
// with its own Adam.  Given the advantages and value targets fixed up front no net reads another one (IPPO.py:254-317; MAPPO.py:391-442
// steps actor and critic of an agent through ONE Adam over both parameter lists, which is elementwise: two Adams with equal settings).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/act_common.hpp"
#include "device/mappo.hpp"

namespace frl {

// the critic's input of agent i: its own observation block, or all blocks (they are contiguous in a record, in agent order)
struct CriticIn { int obs, nobs, width; };
__device__ __forceinline__ CriticIn critic_in(const EngineDesc& D, int i) {
    const RecordDesc& R = D.rec;
    if (D.algo == ALGO_MAPPO) return CriticIn{R.obs_off[0], R.nobs_off[0], R.obs_total};
    return CriticIn{R.obs_off[i], R.nobs_off[i], R.obs_dim[i]};
}

// ---- td_delta_i = r_i + gamma (1 - done_i) V_i(s') - V_i(s) over the horizon (MAPPO.py:366-377, IPPO.py:260-262); grid (chunks, P * n)
__global__ __launch_bounds__(256) void mappo_values_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, u = blockIdx.y, p = u / n, i = u - p * n;
    const int rc = D.rc, r0 = blockIdx.x * rc, T = a.horizon, nv = min(rc, T - r0);
    const NetDesc& N = D.net[2 * i + 1];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    g_cf theta = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[2 * i + 1]);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    const CriticIn ci = critic_in(D, i);
    const int kpad = N.L[0].k_pad;
    float v0 = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        const int src = pass == 0 ? ci.obs : ci.nobs;
        for (int e = threadIdx.x; e < rc * kpad; e += kWG) {
            const int r = e / kpad, c = e - r * kpad;
            S.xin[r * S.xp + c] = (r < nv && c < ci.width) ? ring[(size_t)(r0 + r) * R.stride + src + c] : 0.f;
        }
        __syncthreads();
        mappo_fwd(D, N, theta, S, X, ci.width, ACT_NONE);
        if (threadIdx.x < nv) {
            const float v = S.outb[threadIdx.x * S.op];
            if (pass == 0) {
                v0 = v;
            } else {
                g_cf rec = ring + (size_t)(r0 + threadIdx.x) * R.stride;
                const size_t o = (size_t)u * T + r0 + threadIdx.x;
                a.vs[o] = v0;
                a.td[o] = rec[R.rew_off + i] + a.gamma * (1.f - rec[R.done_off + i]) * v - v0;
                a.advd[o] = rec[R.extra_off + R.act_total + i];
            }
        }
        __syncthreads();
    }
}

// ---- after the scan: v_target = adv + V(s) (MAPPO.py:384, IPPO.py:269) and the optional (adv - mean) / (std + 1e-8) with the unbiased
// std: over the learner's whole [T][n] matrix on MAPPO engines (:385-386), per agent column on IPPO engines (:270-271).  grid (P)
__global__ __launch_bounds__(256) void mappo_adv_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    __shared__ float red_s[8];
    lds_f red = (lds_f)red_s;
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, p = blockIdx.x, T = a.horizon, TN = T * n;
    g_cf seq = as_global(a.adv_seq + (size_t)p * TN);
    g_cf vs = as_global(a.vs + (size_t)p * TN);
    g_f raw = as_global(a.adv_raw + (size_t)p * TN);
    g_f adv = as_global(a.adv + (size_t)p * TN);
    g_f vt = as_global(a.vtarget + (size_t)p * TN);
    for (int e = threadIdx.x; e < TN; e += kWG) {
        const int t = e / n, j = e - t * n;
        const float x = seq[(size_t)j * T + t];
        raw[e] = x;
        adv[e] = x;
        vt[e] = x + vs[(size_t)j * T + t];
    }
    if (!a.adv_norm) return;
    __syncthreads();
    const bool joint = D.algo == ALGO_MAPPO;
    const int groups = joint ? 1 : n, cnt = joint ? TN : T;
    for (int g = 0; g < groups; ++g) {
        // element k of group g: the whole matrix, or column g
        auto at = [&](int k) { return joint ? k : k * n + g; };
        float s1 = 0.f;
        for (int k = threadIdx.x; k < cnt; k += kWG) s1 += raw[at(k)];
        const float mean = block_sum(s1, red) / (float)cnt;
        float s2 = 0.f;
        for (int k = threadIdx.x; k < cnt; k += kWG) { const float d = raw[at(k)] - mean; s2 += d * d; }
        const float sd = sqrtf(block_sum(s2, red) / (float)(cnt - 1));
        for (int k = threadIdx.x; k < cnt; k += kWG) adv[at(k)] = (raw[at(k)] - mean) / (sd + 1e-8f);
    }
}

// ---- all minibatch steps of one net of one (learner, agent); grid (P * n, 2): blockIdx.y 0 = the actor's steps, 1 = the critic's
__global__ __launch_bounds__(256) void mappo_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, u = blockIdx.x, p = u / n, i = u - p * n;
    const int T = a.horizon, mb = a.minibatch, rc = D.rc;
    const bool do_actor = blockIdx.y == 0;
    const int net = 2 * i + (do_actor ? 0 : 1);
    const NetDesc& N = D.net[net];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    const size_t off = (size_t)p * D.learner_stride + D.net_off[net];
    g_f th = as_global(D.theta + off);
    g_f G = as_global(D.grad + off);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_cf adv = as_global(a.adv + (size_t)p * T * n);
    g_cf vt = as_global(a.vtarget + (size_t)p * T * n);
    const bool discrete = D.n_discrete > 0;
    const int c0 = D.algo == ALGO_MAPPO ? 0 : i, c1 = D.algo == ALGO_MAPPO ? n : i + 1;      // advantage / target columns of a row
    const int O = R.obs_dim[i], A = D.net[2 * i].L[2].n;
    const int logp_col = R.extra_off + (R.act_off[i] - R.act_off[0]);                       // the log-prob blocks come first, in agent order
    const CriticIn ci = critic_in(D, i);
    const int npad = N.L[2].n_pad;
    int* steps = D.steps + (size_t)p * (kMaxNets + 1);
    int t_adam = steps[net];
    const int n_mb = (T + mb - 1) / mb;
    float* trace = a.trace + (size_t)u * a.k_epochs * n_mb * 2;
    constexpr float kHalfLog2PiPlusHalf = 1.41893853320467274178f;   // 0.5 + 0.5*log(2*pi)
    LearnArgs la = {};
    la.huber = a.huber;
    la.huber_delta = a.huber_delta;
    float last = 0.f;

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
                if (!discrete && threadIdx.x < A) ent = kHalfLog2PiPlusHalf + clamp_log_std(th[N.extra_off + threadIdx.x]);
                const float ent_sum = block_sum(ent, S.red);          // Normal's entropy: the same for every row
                for (int r0 = 0; r0 < m; r0 += rc) {
                    const int nv = min(rc, m - r0);
                    gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, R.obs_off[i], O, 0);
                    zero_cols(S.xin, S.xp, rc, O, N.L[0].k_pad);
                    __syncthreads();
                    mappo_fwd(D, N, th, S, X, O, discrete ? ACT_NONE : ACT_TANH);          // mean = tanh(mean_layer(.))
                    if (discrete) {
                        // Categorical(probs = softmax(l3)): torch renormalises the probabilities and clamps them to [eps, 1 - eps] before
                        // the logarithm; one thread per row
                        if (threadIdx.x < rc) {
                            const int r = threadIdx.x;
                            if (r < nv) {
                                const int t = idx[r0 + r];
                                g_cf rec = ring + (size_t)t * R.stride;
                                float mx = S.outb[r * S.op];
                                for (int c = 1; c < A; ++c) mx = fmaxf(mx, S.outb[r * S.op + c]);
                                float sum = 0.f;
                                for (int c = 0; c < A; ++c) sum += expf(S.outb[r * S.op + c] - mx);
                                float psum = 0.f;
                                for (int c = 0; c < A; ++c) psum += expf(S.outb[r * S.op + c] - mx) / sum;
                                const int ar = (int)rec[R.act_off[i]];
                                auto logp_of = [&](float pc) { return logf(fminf(fmaxf(pc / psum, 1.1920929e-07f), 1.f - 1.1920929e-07f)); };
                                float entr = 0.f, lp_now = 0.f;
                                for (int c = 0; c < A; ++c) {
                                    const float pc = expf(S.outb[r * S.op + c] - mx) / sum;
                                    const float lg = logp_of(pc);
                                    entr -= lg * pc;
                                    if (c == ar) lp_now = lg;
                                }
                                const float ratio = expf(lp_now - rec[logp_col]);
                                const float coef = surrogate_row(ratio, adv + (size_t)t * n, c0, c1, a.clip, lossp) * invmn;
                                entp += entr;
                                for (int c = 0; c < npad; ++c) {
                                    float d = 0.f;
                                    if (c < A) {
                                        const float pc = expf(S.outb[r * S.op + c] - mx) / sum;
                                        d = coef * ((c == ar ? 1.f : 0.f) - pc) + (a.ent_coef * invm) * pc * (logp_of(pc) + entr);
                                    }
                                    S.abuf[r * S.ap + c] = d;      // staged: outb is still being read by this row
                                }
                            } else {
                                for (int c = 0; c < npad; ++c) S.abuf[r * S.ap + c] = 0.f;
                            }
                            for (int c = 0; c < npad; ++c) S.outb[r * S.op + c] = S.abuf[r * S.ap + c];
                        }
                        __syncthreads();
                    } else {
                        if (threadIdx.x < rc) {
                            const int r = threadIdx.x;
                            float coef = 0.f;
                            if (r < nv) {
                                const int t = idx[r0 + r];
                                g_cf rec = ring + (size_t)t * R.stride;
                                float lp_now = 0.f, lp_old = 0.f;
                                for (int c = 0; c < A; ++c) {
                                    const float ls = clamp_log_std(th[N.extra_off + c]);
                                    lp_now += normal_logp(rec[R.act_off[i] + c] - S.outb[r * S.op + c], expf(ls), ls);
                                    lp_old += rec[logp_col + c];
                                }
                                coef = surrogate_row(expf(lp_now - lp_old), adv + (size_t)t * n, c0, c1, a.clip, lossp) * invmn;
                            }
                            S.dabuf[r * S.ap] = coef;      // d loss / d sum_c logp_now
                        }
                        __syncthreads();
                        for (int e = threadIdx.x; e < rc * npad; e += kWG) {
                            const int r = e / npad, c = e - r * npad;
                            float d = 0.f, dl = 0.f;
                            if (r < nv && c < A) {
                                const float coef = S.dabuf[r * S.ap];
                                const float mean = S.outb[r * S.op + c];
                                const float var = expf(2.f * clamp_log_std(th[N.extra_off + c]));
                                const float dm = ring[(size_t)idx[r0 + r] * R.stride + R.act_off[i] + c] - mean;
                                d = coef * dm / var * (1.f - mean * mean);        // through mean = tanh(z)
                                dl = coef * (dm * dm / var - 1.f);
                            }
                            S.outb[r * S.op + c] = d;
                            if (c < A) S.abuf[r * S.ap + c] = dl;
                        }
                        __syncthreads();
                        if (threadIdx.x < A)
                            for (int r = 0; r < rc; ++r) gls += S.abuf[r * S.ap + threadIdx.x];
                    }
                    mappo_bwd(D, N, th, G, S, X, r0 == 0 ? GS_STORE : GS_ADD);
                }
                if (!discrete && threadIdx.x < A)
                    G[N.extra_off + threadIdx.x] = log_std_grad_open(th[N.extra_off + threadIdx.x]) ? (gls - a.ent_coef) : 0.f;
                const float surr = block_sum(lossp, S.red) * invmn;
                const float entm = discrete ? block_sum(entp, S.red) * invm : ent_sum;
                loss = surr - a.ent_coef * entm;
            } else {
                // ---------------- critic: the loss of v_target[idx] against V (MAPPO.py:416-436, IPPO.py:300-316)
                float lossp = 0.f;
                for (int r0 = 0; r0 < m; r0 += rc) {
                    const int nv = min(rc, m - r0);
                    gather_cols(S.xin, S.xp, rc, nv, idx + r0, ring, R.stride, ci.obs, ci.width, 0);
                    zero_cols(S.xin, S.xp, rc, ci.width, N.L[0].k_pad);
                    __syncthreads();
                    mappo_fwd(D, N, th, S, X, ci.width, ACT_NONE);
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

// ---- frl_act on these engines: kernels_act.hip's act_kernel with the normalised forward in front of the shared epilogue
__global__ __launch_bounds__(256) void mappo_act_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc;
    const NetDesc& N = D.net[a.net];
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    const int rc = D.rc, nv = min(rc, a.n_rows - r0);
    g_cf theta = as_global((a.use_target ? D.target : D.theta) + (size_t)p * D.learner_stride + D.net_off[a.net]);
    const int K = a.in_dim, kpad = N.L[0].k_pad;
    g_cf in = as_global(a.in + ((size_t)p * a.n_rows + r0) * K);
    for (int e = threadIdx.x; e < rc * kpad; e += kWG) {
        const int r = e / kpad, c = e - r * kpad;
        S.xin[r * S.xp + c] = (r < nv && c < K) ? in[(size_t)r * K + c] : 0.f;
    }
    __syncthreads();
    const int out_act = (a.mode == ACTM_TANH || a.mode == ACTM_PPO_SAMPLE) ? ACT_TANH : ACT_NONE;
    mappo_fwd(D, N, theta, S, X, K, out_act);
    act_epilogue(D, a, N, theta, S.outb, S.op, nv, r0, p, N.L[2].n);
}

}  // namespace frl
