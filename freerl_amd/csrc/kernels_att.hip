// ATT-MADDPG (MADDPG_file/MADDPG_simple_with_tricks.py:178-199 with trick['ATT'], ATT.py:181-229): the gradient kernels of an
// ALGO_MADDPG_ATT engine and the critic's forward for frl_act.  The row-chunk skeleton of kernels_critic.hip / kernels_actor.hip — a unit =
// (learner, agent), a workgroup walks `cps` chunks of kAttRc rows and leaves one gradient slab, reduce + clip + Adam and the soft updates
// are kernels_update.hip's — around the attention critic of device/att.hpp.
#include <hip/hip_runtime.h>

#include "device/att.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// x_e's observation block and x_d from ring rows: every agent's (next) observation into xin[:, 0:OT), the stored actions of the other agents
// into xd.  own_act: also the agent's own stored action into xin[:, OT:OT+Aa) (the critic step); else the caller places it.
__device__ __forceinline__ void att_gather_stored(const EngineDesc& D, const Lds& S, const AttLds& A, const NetDesc& NC, int ag, int nv, g_ci idx, g_cf ring,
                                                  bool own_act) {
    const RecordDesc& R = D.rec;
    const int rc = S.rc, OT = R.obs_total, AT = R.act_total, Aa = R.act_dim[ag], a0 = R.act_off[ag] - R.act_off[0];
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], OT, 0);
    if (own_act) gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.act_off[ag], Aa, OT);
    zero_cols(S.xin, S.xp, rc, OT + Aa, NC.L[ATT_E].k_pad);
    if (a0 > 0) gather_cols(A.xd, A.dp, rc, nv, idx, ring, R.stride, R.act_off[0], a0, 0);
    if (AT - a0 - Aa > 0) gather_cols(A.xd, A.dp, rc, nv, idx, ring, R.stride, R.act_off[ag] + Aa, AT - a0 - Aa, a0);
    zero_cols(A.xd, A.dp, rc, AT - Aa, NC.L[ATT_D].k_pad);
}

// ------------------------------------------------------------------------------------- critic
// T = r_i + gamma critic_target_i(o', actor_target_j(o'_j) for all j) (1 - done_i); mse(critic_i(o, a), T); backward -> slab.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void att_critic_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = agent_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int n = D.n_agents, p = U.p, ag = U.ag, sl = U.sl;
    const RecordDesc& R = D.rec;
    const NetDesc& NC = D.net[2 * ag + 1];
    const Lds S = carve(D, smem);
    const AttLds A = carve_att(D, S, smem);
    const int rc = D.rc, B = a.batch;
    const ChunkRange cr = chunk_range(D, B, sl);
    g_cf thC = U.theta(2 * ag + 1);
    g_cf tgC = U.target(2 * ag + 1);
    g_f slab = U.slab(2 * ag + 1);
    g_cf ring = U.ring();
    const int OT = R.obs_total, AT = R.act_total, Aa = R.act_dim[ag], a0 = R.act_off[ag] - R.act_off[0];
    const float invB = 1.f / (float)B;

    float lossp = 0.f;
    for (int ck = cr.c0; ck < cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const bool first = (ck == cr.c0);
    const int gs = first ? (D.cps > 1 ? GS_STORE : GS_STREAM) : GS_ADD;
    const int r0 = ck * rc, nv = min(rc, B - r0);
    g_ci idx = U.idx(r0);
    if (!first) lds_barrier();
    // ---- a'_j = actor_target_j(o'_j) for every agent j (MADDPG_simple_with_tricks.py:168), all agents' columns of abuf
    for (int j = 0; j < n; ++j) {
        const NetDesc& NJ = D.net[2 * j];
        g_cf tgJ = U.target(2 * j);
        const int Oj = R.obs_dim[j], Aj = R.act_dim[j], cj = R.act_off[j] - R.act_off[0];
        gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[j], Oj, 0);
        zero_cols(S.xin, S.xp, rc, Oj, NJ.L[0].k_pad);
        FRL_PHASE(S);
        mlp_fwd_rows(NJ, 0, NJ.n_layers, tgJ, S, ACT_TANH, [&](int r) {
            for (int c = 0; c < Aj; ++c) S.abuf[r * S.ap + cj + c] = S.outb[r * S.op + c];
        });
    }
    // ---- the target critic on x_e = [o'_all | a'_i], x_d = a'_{j != i}
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], OT, 0);
    for (int e = threadIdx.x; e < rc * Aa; e += kWG) {
        const int r = e / Aa, c = e - r * Aa;
        S.xin[r * S.xp + OT + c] = S.abuf[r * S.ap + a0 + c];
    }
    zero_cols(S.xin, S.xp, rc, OT + Aa, NC.L[ATT_E].k_pad);
    att_fill_xd(A, rc, S.abuf, S.ap, a0, Aa, AT, NC.L[ATT_D].k_pad);
    FRL_PHASE(S);
    att_fwd(NC, tgC, S, A);
    if (threadIdx.x < nv) {
        g_cf rec = ring + (size_t)idx[threadIdx.x] * R.stride;
        S.y[threadIdx.x] = td_target(rec[R.rew_off + ag], rec[R.done_off + ag], a.gamma, S.outb[threadIdx.x * S.op]);
    }
    // ---- the online critic on the stored row: forward, MSE delta, backward (nothing below reads outb before att_fwd rewrites it)
    att_gather_stored(D, S, A, NC, ag, nv, idx, ring, true);
    FRL_PHASE(S);
    att_fwd(NC, thC, S, A);
    const int npad = NC.L[ATT_FC2].n_pad;
    if (threadIdx.x < rc) {
        const int r = threadIdx.x;
        lds_f o = S.outb + r * S.op;
        float d = 0.f;
        if (r < nv) {
            float lrow, grow;
            td_loss_row(a, o[0] - S.y[r], lrow, grow);
            d = grow * invB;
            lossp += lrow;
        }
        o[0] = d;
        for (int c = 1; c < npad; ++c) o[c] = 0.f;
    }
    FRL_PHASE(S);
    att_bwd(NC, thC, slab, S, A, gs, false, 0, 0);
    }
    store_loss_part(U, S, lossp);
}

// -------------------------------------------------------------------------------------- actor
// a_i = actor_i(o_i); loss = -mean critic_i(o, [a_j stored, a_i]) through the critic the critic Adam has just stepped; dQ/da_i out of a
// dX-only backward down the encoder branch (no critic gradient reaches the slab); actor backward -> slab.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void att_actor_kernel(const EngineDesc* __restrict__ Dp, LearnArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = agent_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const int n = D.n_agents, p = U.p, ag = U.ag, sl = U.sl;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[2 * ag];
    const NetDesc& NC = D.net[2 * ag + 1];
    const Lds S = carve(D, smem);
    const AttLds A = carve_att(D, S, smem);
    const int rc = D.rc, B = a.batch;
    const ChunkRange cr = chunk_range(D, B, sl);
    g_cf thA = U.theta(2 * ag);
    g_cf thC = U.theta(2 * ag + 1);
    g_f slab = U.slab(2 * ag);
    g_cf ring = U.ring();
    const int OT = R.obs_total, Oa = R.obs_dim[ag], Aa = R.act_dim[ag];
    const float invB = 1.f / (float)B;
    const int ct0 = OT / 16, ct1 = (OT + Aa + 15) / 16;      // the own-action columns of x_e: OT .. OT + Aa - 1

    float alossp = 0.f;
    for (int ck = cr.c0; ck < cr.c1; ++ck) {
    const bool first = (ck == cr.c0);
    const int gs = first ? (D.cps > 1 ? GS_STORE : GS_STREAM) : GS_ADD;
    const int r0 = ck * rc, nv = min(rc, B - r0);
    g_ci idx = U.idx(r0);
    if (!first) lds_barrier();
    // -- a = actor(obs); its hidden rows parked in act_spill while the critic pass reuses h1 / h2 (as ac_actor_kernel does)
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[ag], Oa, 0);
    zero_cols(S.xin, S.xp, rc, Oa, NA.L[0].k_pad);
    FRL_PHASE(S);
    const int spill_n4 = 2 * rc * S.hp / 4;                 // h1 | h2, adjacent in LDS: act_spill_pitch(D) floats (rc = D.rc, S.hp = hidden_pitch(D.hidden))
    FRL_GLB f32x4* spill = U.spill();
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_TANH, [&](int r) {
        for (int c = 0; c < Aa; ++c) S.abuf[r * S.ap + c] = S.outb[r * S.op + c];
    }, [&]() {
        for (int i = threadIdx.x; i < spill_n4; i += kWG) spill[i] = ld4((lds_cf)(S.h1 + 4 * i));
    });
    // -- Q(o, [a_j stored, a_i = actor_i(o_i)]) and dQ/da_i
    att_gather_stored(D, S, A, NC, ag, nv, idx, ring, false);
    for (int e = threadIdx.x; e < rc * Aa; e += kWG) {
        const int r = e / Aa, c = e - r * Aa;
        S.xin[r * S.xp + OT + c] = S.abuf[r * S.ap + c];
    }
    FRL_PHASE(S);
    att_fwd(NC, thC, S, A);
    const int npad = NC.L[ATT_FC2].n_pad;
    if (threadIdx.x < rc) {
        const int r = threadIdx.x;
        lds_f o = S.outb + r * S.op;
        if (r < nv) alossp += -o[0];
        o[0] = (r < nv) ? -invB : 0.f;
        for (int c = 1; c < npad; ++c) o[c] = 0.f;
    }
    FRL_PHASE(S);
    att_bwd(NC, thC, nullptr, S, A, GS_ADD, true, ct0, ct1);
    for (int e = threadIdx.x; e < rc * Aa; e += kWG) {
        const int r = e / Aa, c = e - r * Aa;
        S.dabuf[r * S.ap + c] = S.xin[r * S.xp + OT + c];
    }
    FRL_PHASE(S);
    // -- the actor's activations back (same thread, same addresses as the spill), its input back in xin, the head delta through tanh
    for (int i = threadIdx.x; i < spill_n4; i += kWG) st4(S.h1 + 4 * i, spill[i]);
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[ag], Oa, 0);
    zero_cols(S.xin, S.xp, rc, Oa, NA.L[0].k_pad);
    const int napad = NA.L[NA.n_layers - 1].n_pad;
    for (int e = threadIdx.x; e < rc * napad; e += kWG) {
        const int r = e / napad, c = e - r * napad;
        S.outb[r * S.op + c] = (r < nv && c < Aa) ? tanh_delta(S.dabuf[r * S.ap + c], S.abuf[r * S.ap + c]) : 0.f;
    }
    FRL_PHASE(S);
    mlp_bwd(NA, 0, NA.n_layers, thA, slab, S, gs, false, 0, 0);
    }
    const float la = block_sum(alossp, S.red);
    store_loss_parts(U, la, 0.f);
}

// ------------------------------------------------------------------------------------ forward
// frl_act on net 2i+1 (FRL_ACT_RAW): Q of rows [all obs | all actions] from the online or the target critic.  grid = (row chunks, learners).
__global__ __launch_bounds__(256) void att_q_kernel(const EngineDesc* __restrict__ Dp, ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.y, r0 = blockIdx.x * D.rc;
    const RecordDesc& R = D.rec;
    const int ag = a.net / 2;
    const NetDesc& NC = D.net[a.net];
    const Lds S = carve(D, smem);
    const AttLds A = carve_att(D, S, smem);
    const int rc = D.rc, nv = min(rc, a.n_rows - r0);
    const int OT = R.obs_total, AT = R.act_total, Aa = R.act_dim[ag], a0 = R.act_off[ag] - R.act_off[0], K = OT + AT;
    g_cf theta = as_global((a.use_target ? D.target : D.theta) + (size_t)p * D.learner_stride + D.net_off[a.net]);
    g_cf in = as_global(a.in + ((size_t)p * a.n_rows + r0) * K);
    const int ke = NC.L[ATT_E].k_pad, kd = NC.L[ATT_D].k_pad;
    for (int e = threadIdx.x; e < rc * ke; e += kWG) {
        const int r = e / ke, c = e - r * ke;
        float v = 0.f;
        if (r < nv && c < OT + Aa) v = in[(size_t)r * K + (c < OT ? c : c + a0)];
        S.xin[r * S.xp + c] = v;
    }
    for (int e = threadIdx.x; e < rc * kd; e += kWG) {
        const int r = e / kd, c = e - r * kd;
        float v = 0.f;
        if (r < nv && c < AT - Aa) v = in[(size_t)r * K + OT + (c < a0 ? c : c + Aa)];
        A.xd[r * A.dp + c] = v;
    }
    __syncthreads();
    att_fwd(NC, theta, S, A);
    if (threadIdx.x < nv) a.out[(size_t)p * a.n_rows + r0 + threadIdx.x] = S.outb[threadIdx.x * S.op];
}

}  // namespace frl
