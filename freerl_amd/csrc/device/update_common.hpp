// The skeleton shared by the row-chunk gradient kernels (kernels_dqn / _c51 / _critic / _actor / _sacd / _reinforce / _envelope /
// _envelope_ddpg / _gail / _att / _masac .hip): LDS carve from the engine descriptor, block id -> the unit a workgroup works for, the
// row chunks it walks, and the passes more than one of those kernels run.  Every address comes from ../rowchunk_layout.h, which
// tests/engine_plan_probe.cpp walks against the plan's buffer sizes on the CPU; a kernel writes only what differs from the others.
// (The arithmetic of the policies and TD targets is in policy.hpp.)
#pragma once
#include "net.hpp"

namespace frl {

__device__ __forceinline__ Lds carve(const EngineDesc& D, float* smem) {
    return carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
}

// The unit of one workgroup: learner p, agent ag, slice sl (its slab and its `cps` row chunks).  block id -> (unit, slice): the `ns`
// slices of unit u sit on blocks {8*ns*g + x + 8s}, i.e. all on XCD x and adjacent in dispatch order.
struct UnitChunk { bool first; int gs, r0, nv; g_ci idx; g_cf noise; };
// The chunks of one workgroup, set up once ahead of the loop `for (int ck = W.cr.c0; ck < W.cr.c1; ++ck)`
struct RowWalk {
    ChunkRange cr;
    g_ci idx0;          // the unit's idx and noise (draw set 0; set k lies k * noise_set_floats further) at row 0
    g_cf noise0;
    int act_max;
    // chunk ck: its rows and store mode, idx and noise advanced to its first row, then the barrier between two chunks
    __device__ __forceinline__ UnitChunk chunk(int ck) const {
        const RowChunk c = row_chunk(cr, ck);
        const UnitChunk uc{c.first, c.gs, c.r0, c.nv, idx0 + c.r0, noise0 + (size_t)c.r0 * act_max};
        if (!c.first) lds_barrier();
        return uc;
    }
};
struct RowUnit {
    const EngineDesc& D;
    int p, ag, sl;
    bool none;          // the 8-aligned grid's spare workgroups: no unit, return at once

    __device__ __forceinline__ size_t lbase() const { return (size_t)p * D.learner_stride; }
    __device__ __forceinline__ g_cf theta(int net) const { return as_global(D.theta + lbase() + D.net_off[net]); }
    __device__ __forceinline__ g_cf target(int net) const { return as_global(D.target + lbase() + D.net_off[net]); }
    __device__ __forceinline__ g_f slab(int net) const { return as_global(D.slab + slab_offset(D, p, sl, net)); }
    __device__ __forceinline__ g_cf ring() const { return as_global(D.replay + (size_t)p * D.capacity * D.rec.stride); }
    __device__ __forceinline__ float* part() const { return D.part + part_offset(D, p, ag, sl); }
    __device__ __forceinline__ g_ci idx(int r0) const { return as_global_i(D.idx + idx_offset(D, p, ag, r0)); }
    __device__ __forceinline__ g_cf noise(int set, int r0) const { return as_global(D.noise + noise_offset(D, p, ag, set, r0)); }
    __device__ __forceinline__ FRL_GLB f32x4* spill() const { return (FRL_GLB f32x4*)(D.act_spill + act_spill_offset(D, p, ag, sl)); }
    __device__ __forceinline__ RowWalk walk(int rows, bool rereads_slab = false) const {
        return RowWalk{chunk_range(D, rows, sl, rereads_slab), idx(0), noise(0, 0), D.act_max};
    }
};
// units = the learners [p0, p0 + p_count), all for agent `ag` (single-agent engines: 0)
__device__ __forceinline__ RowUnit learner_unit(const EngineDesc& D, int ns, int p0, int p_count, int ag = 0) {
    const int group = 8 * ns, g = blockIdx.x / group, l = blockIdx.x - g * group, unit = g * 8 + (l & 7);
    return RowUnit{D, p0 + unit, ag, l >> 3, unit >= p_count};
}
// units = the (learner, agent) pairs of those learners
__device__ __forceinline__ RowUnit agent_unit(const EngineDesc& D, int ns, int p0, int p_count) {
    const int group = 8 * ns, g = blockIdx.x / group, l = blockIdx.x - g * group, unit = g * 8 + (l & 7), n = D.n_agents;
    return RowUnit{D, p0 + unit / n, unit % n, l >> 3, unit >= p_count * n};
}

// ------------------------------------------------------------------------------ passes shared by several kernels
// the joint critic input's action block: columns [OT, OT + AT) of xin from abuf, zero up to the first layer's k_pad
__device__ __forceinline__ void joint_actions_to_xin(const Lds& S, int OT, int AT, int k_pad) {
    for (int e = threadIdx.x; e < S.rc * AT; e += kWG) {
        const int r = e / AT, c = e - r * AT;
        S.xin[r * S.xp + OT + c] = S.abuf[r * S.ap + c];
    }
    zero_cols(S.xin, S.xp, S.rc, OT + AT, k_pad);
}

// min over the target critic's heads of Q(xin) for row threadIdx.x (one head: its value): both heads in three phases where the net
// allows it, else head by head
__device__ __forceinline__ float target_q_min(const NetDesc& NC, g_cf tgC, const Lds& S) {
    const int rc = S.rc, ql = NC.n_layers / NC.heads;
    float q = 0.f;
    if (twin_target_fusable(NC)) {
        twin_target_fwd(NC, tgC, S);
        if (threadIdx.x < rc) q = fminf(twin_target_q(NC, tgC, S, threadIdx.x, 0), twin_target_q(NC, tgC, S, threadIdx.x, 1));
    } else {
        mlp_fwd(NC, 0, ql, tgC, S, ACT_NONE);
        if (threadIdx.x < rc) q = S.outb[threadIdx.x * S.op];
        if (NC.heads == 2) {
            FRL_PHASE(S);
            mlp_fwd(NC, ql, ql, tgC, S, ACT_NONE);
            if (threadIdx.x < rc) q = fminf(q, S.outb[threadIdx.x * S.op]);
        }
    }
    return q;
}

// the online critic heads on the [obs | act] rows already in xin (both heads read the same rows: nothing in between writes xin):
// forward, the TD loss's delta against S.y in the finalize phase, backward -> slab.  lossp: the thread's running loss sum
__device__ __forceinline__ void critic_heads_td(const NetDesc& NC, g_cf thC, g_f slab, const Lds& S, const LearnArgs& a, int nv, int gs, float invB,
                                                float& lossp) {
    const int heads = NC.heads, ql = NC.n_layers / heads;
    for (int h = 0; h < heads; ++h) {
        FRL_PHASE(S);
        const int npad = NC.L[h * ql + ql - 1].n_pad;
        mlp_fwd_rows(NC, h * ql, ql, thC, S, ACT_NONE, [&](int r) {
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
        });
        mlp_bwd(NC, h * ql, ql, thC, slab, S, gs, false, 0, 0);
    }
}

// the actor's hidden activations (h1 | h2, adjacent in LDS) parked in the unit's act_spill block while a critic pass reuses them, and
// back: same thread, same addresses both ways.  A second actor forward cost 16 % of ac_actor_kernel (tools/phase_timing.py actor).
// The floats copied, 2 * S.rc * S.hp, ARE act_spill_pitch(D): carve() sets S.rc = D.rc and S.hp = hidden_pitch(D.hidden), the two factors
// of the layout's pitch (taken from the carve the kernel holds: reading D again inside the chunk loop costs the kernels registers)
__device__ __forceinline__ void park_hidden(const Lds& S, FRL_GLB f32x4* spill) {
    for (int i = threadIdx.x; i < 2 * S.rc * S.hp / 4; i += kWG) spill[i] = ld4((lds_cf)(S.h1 + 4 * i));
}
__device__ __forceinline__ void restore_hidden(const Lds& S, FRL_GLB f32x4* spill) {
    for (int i = threadIdx.x; i < 2 * S.rc * S.hp / 4; i += kWG) st4(S.h1 + 4 * i, spill[i]);
}

// the workgroup's loss partials -> its part slot
__device__ __forceinline__ void store_loss_part(const RowUnit& U, const Lds& S, float lossp) {
    const float ls = block_sum(lossp, S.red);
    if (threadIdx.x == 0) U.part()[0] = ls;
}
__device__ __forceinline__ void store_loss_parts(const RowUnit& U, float loss, float entropy) {      // (already summed over the block)
    if (threadIdx.x == 0) {
        float* pt = U.part();
        pt[0] = loss;
        pt[1] = entropy;
    }
}

}  // namespace frl
