// CEM_GD3PG's pieces of the row-chunk skeleton (kernels_cem_gd3pg.hip; CEM_GD3PG_file/CEM_GD3PG.py): the net numbering, which actor a
// learner's call guides, the (learner, actor) unit of the actor launch and the batch-global KL.  Every address comes from
// ../rowchunk_layout.h (tests/cem_gd3pg_plan_probe.cpp walks them against the plan's buffer sizes on the CPU).
#pragma once
#include "update_common.hpp"

namespace frl {

enum CemNet : int { CEM_ACTOR_1 = 0, CEM_ACTOR_2 = 1, CEM_CRITIC = 2, CEM_DOMAIN = 3 };
constexpr int kCemOut = 8;      // floats per learner of EngineDesc::cem_out (frl_cem_gd3pg_args::out)
enum CemOut : int { CEM_OUT_CRITIC_LOSS = 0, CEM_OUT_CRITIC_NORM = 1, CEM_OUT_ACTOR_LOSS = 2, CEM_OUT_ACTOR_NORM = 3 /* + 2 actor */, CEM_OUT_KL = 6, CEM_OUT_ROWS = 7 };

// EngineDesc::cem_ctl [2][P]: is_F1_more, then delta
__device__ __forceinline__ bool cem_f1_more(const EngineDesc& D, int p) { return D.cem_ctl[p] != 0.f; }
__device__ __forceinline__ float cem_delta(const EngineDesc& D, int p) { return D.cem_ctl[D.P + p]; }
// the guided actor of learner p: actor_2 when F1 did better (:201-208), else actor_1 (:209-216)
__device__ __forceinline__ int cem_guided(const EngineDesc& D, int p) { return cem_f1_more(D, p) ? CEM_ACTOR_2 : CEM_ACTOR_1; }

// The actor launch: 2 p_count units on learner_unit's grid, unit u = (learner p0 + u / 2, actor u % 2).  The RowUnit is the LEARNER's
// (ag = 0: its idx, its part slots, its slice's slab), `actor` picks the net and the spill block
__device__ __forceinline__ RowUnit cem_actor_unit(const EngineDesc& D, int ns, int p0, int p_count, int& actor) {
    const RowUnit V = learner_unit(D, ns, 0, kCemActors * p_count);
    actor = V.p % kCemActors;
    return RowUnit{D, p0 + V.p / kCemActors, 0, V.sl, V.none};
}
__device__ __forceinline__ FRL_GLB f32x4* cem_spill(const RowUnit& U, int actor) {
    return (FRL_GLB f32x4*)(U.D.act_spill + cem_spill_offset(U.D, U.p, actor, U.sl));
}
// the domain actor's rows of chunk r0 .. (pitch act_max), written by the critic launch and read by the guided actor's workgroups
__device__ __forceinline__ g_f cem_domain_rows(const RowUnit& U, int r0) { return as_global(U.D.noise + cem_domain_offset(U.D, U.p, r0)); }

// sum c^2 over the whole batch: the critic launch's workgroups left their partial sums in their part slots; every reader adds them in
// slice order, so that all workgroups of a learner (and cem_step_kernel) see the same bits
__device__ __forceinline__ float cem_c2_sum(const EngineDesc& D, int p, int ns) {
    const float* pt = D.part + part_offset(D, p, 0, 0);
    float s = 0.f;
    for (int k = 0; k < ns; ++k) s += pt[kPartFloats * k + CEM_PART_C2];
    return s;
}
// KL = sqrt(sum c^2 / B) (:206); 0 where torch's sqrt backward would give NaN
__device__ __forceinline__ float cem_kl(float c2, int B) { return c2 > 0.f ? sqrtf(c2 / (float)B) : 0.f; }

}  // namespace frl
