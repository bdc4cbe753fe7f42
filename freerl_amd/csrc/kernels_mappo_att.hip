// MAPPO_attention (MAPPO_file/MAPPO_attention.py:245-404 with improvement['attention']; attention.py:85-205): MAPPO's record, actors, GAE
// scan and advantage launch, but every critic is an Attention_Critic over ONE attention block that all critics of a learner share, and
// the agents are the OUTER loop of learn(): agent i takes all its K_epochs x minibatch steps before agent i+1 starts.  One learn() is
//     mappo_att_values_kernel -> gae_dense_kernel -> mappo_adv_kernel -> mappo_att_update_kernel x n_agents (agent 0, 1, ..)
// The dependency between agents — critic i+1 starts from the attention block as critic i's last step left it — is carried by stream
// order between the launches and by nothing else: launch i writes actor i, critic i's own layers, moments and gradient, and the
// attention block in net 1's copy; no workgroup reads what another workgroup of its own launch writes (the actor's workgroup touches
// net 2i only, and with P learners a workgroup stays inside its learner's stride).  The critic's chunk arithmetic, with the streamed
// others and the online softmax, is device/mappo_att.hpp's.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/act_common.hpp"
#include "device/mappo_att.hpp"

namespace frl {

// ---- td_delta_i, V_i(s) and the adv_done column over the horizon, into the slots mappo_values_kernel fills; grid (chunks, P * n)
__global__ __launch_bounds__(256) void mappo_att_values_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int n = D.n_agents, u = blockIdx.y, p = u / n, i = u - p * n;
    const int rc = D.rc, r0 = blockIdx.x * rc, T = a.horizon;
    const NetDesc& N = D.net[2 * i + 1];
    const RecordDesc& R = D.rec;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    const MattLds A = carve_matt(S, D.n_agents);
    g_cf thC = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[2 * i + 1]);
    g_cf thA = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[1]);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    const MattRows rows = {ring, nullptr, r0, R.stride, min(rc, T - r0)};
    float v0 = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        matt_fwd(D, N, thC, thA, S, X, A, rows, pass == 0 ? R.obs_off[0] : R.nobs_off[0], i);
        if (threadIdx.x < rows.nv) {
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

// ---- agent `agent` of every learner; grid (P, 2): blockIdx.y 0 = all steps of its actor (MAPPO's, device/mappo.hpp), 1 = all steps of
// its critic, a persistent workgroup
__global__ __launch_bounds__(256) void mappo_att_update_kernel(const EngineDesc* __restrict__ Dp, MappoArgs a, int agent, float* norm_trace) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x;
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    if (blockIdx.y == 0) mappo_steps<false>(D, a, S, X, p, agent, true, nullptr);
    else matt_critic_steps(D, a, S, X, carve_matt(S, D.n_agents), p, agent, norm_trace);
}

// ---- frl_act with FRL_ACT_RAW on net 2i+1: V_i of dense rows [obs_0 | .. | obs_{n-1}]; grid (chunks, P)
__global__ __launch_bounds__(256) void mappo_att_v_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc, K = a.in_dim;
    const NetDesc& N = D.net[a.net];
    const Lds S = carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
    const MappoLds X = carve_mappo(S);
    g_cf thC = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[a.net]);
    g_cf thA = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[1]);
    const int nv = min(D.rc, a.n_rows - r0);
    const MattRows rows = {as_global(a.in + (size_t)p * a.n_rows * K), nullptr, r0, K, nv};
    matt_fwd(D, N, thC, thA, S, X, carve_matt(S, D.n_agents), rows, 0, a.net / 2);
    act_epilogue(D, a, N, thC, S.outb, S.op, nv, r0, p, 1);
}

}  // namespace frl
