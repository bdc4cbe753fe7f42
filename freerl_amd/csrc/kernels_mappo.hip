// MAPPO and IPPO (MAPPO_file/MAPPO.py:357-482, IPPO.py:252-322): per agent i an actor on its own observation (net 2i) and a critic
// (net 2i+1) on its own observation (IPPO) or on the concatenation of every agent's (MAPPO; HAPPO engines too, whose first three
// launches are this file's: kernels_happo.hip).  One learn() is
//     mappo_values_kernel -> gae_dense_kernel -> mappo_adv_kernel -> mappo_update_kernel
// and the update is ppo_update_kernel's shape: one persistent workgroup per (learner, agent, net) runs all K_epochs x minibatch steps
// with its own Adam.  Given the advantages and value targets fixed up front no net reads another one (IPPO.py:254-317; MAPPO.py:391-442
// steps actor and critic of an agent through ONE Adam over both parameter lists, which is elementwise: two Adams with equal settings).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/act_common.hpp"
#include "device/mappo.hpp"

namespace frl {

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
        load_rows(S.xin, S.xp, rc, nv, ring, r0, R.stride, src, ci.width, kpad);
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
// std: over the learner's whole [T][n] matrix on MAPPO and HAPPO engines (:385-386), per agent column on IPPO engines (:270-271).  grid (P)
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
    const bool joint = mappo_joint(D.algo);
    const int groups = joint ? 1 : n, cnt = joint ? TN : T;
    for (int g = 0; g < groups; ++g) {
        // element k of group g: the whole matrix, or column g
        auto at = [&](int k) { return joint ? k : k * n + g; };
        float s1 = 0.f;
        for (int k = threadIdx.x; k < cnt; k += kWG) s1 += raw[at(k)];
        normalize_adv(s1, cnt, raw, adv, at, red);
    }
}

// ---- all minibatch steps of one net of one (learner, agent); grid (P * n, 2): blockIdx.y 0 = the actor's steps, 1 = the critic's.
// The step loop is device/mappo.hpp's mappo_steps(), which kernels_happo.hip runs too, there with a factor per row
__global__ __launch_bounds__(256) void mappo_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x / D.n_agents, i = blockIdx.x - p * D.n_agents;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    mappo_steps<false>(D, a, S, carve_mappo(S), p, i, blockIdx.y == 0, nullptr);
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
    load_rows(S.xin, S.xp, rc, nv, in, 0, K, 0, K, kpad);
    __syncthreads();
    const int out_act = (a.mode == ACTM_TANH || a.mode == ACTM_PPO_SAMPLE) ? ACT_TANH : ACT_NONE;
    mappo_fwd(D, N, theta, S, X, K, out_act);
    act_epilogue(D, a, N, theta, S.outb, S.op, nv, r0, p, N.L[2].n);
}

}  // namespace frl
