// The row-chunk launch shape in one place: which row chunks a gradient workgroup walks and where its (learner, agent, slice) keeps its
// slab, loss partials, sampled indices, noise draws and parked activations.  Plain C++17 (no HIP): the kernels (device/update_common.hpp),
// the engine plan's buffer counts (engine_plan.hpp) and tests/engine_plan_probe.cpp, which walks every (unit, slice, chunk) against
// those counts on the CPU, all read the same functions.  Single-agent engines are the n_agents == 1, ag == 0 case of every formula.
#pragma once
#include <stddef.h>

#include "frl_desc.h"

#if defined(__HIPCC__)
#define FRL_LAYOUT_FN __host__ __device__ __forceinline__
#else
#define FRL_LAYOUT_FN inline
#endif

namespace frl {

// How a gradient tile reaches its slab: GS_STREAM the slab is written once and read once by reduce_kernel (non-temporal
// store), GS_STORE first of several row chunks (plain store: the next chunk reads it back), GS_ADD a later chunk.
enum GradStore : int { GS_STREAM = 0, GS_STORE = 1, GS_ADD = 2 };

// ------------------------------------------------------------------------------ rows -> chunks -> slices
// A unit's `rows` fall into chunks of rc rows; a workgroup (slice sl of the unit) owns `cps` consecutive chunks (the plan picks cps so
// that one round of workgroups fills the chip): its first chunk stores its weight gradients in the workgroup's slab, the others add
// to them — one slab per workgroup instead of one per chunk for reduce_kernel to stream.
FRL_LAYOUT_FN int rowchunk_chunks(const EngineDesc& D, int rows) { return (rows + D.rc - 1) / D.rc; }
FRL_LAYOUT_FN int rowchunk_ns(const EngineDesc& D, int rows) { return (rowchunk_chunks(D, rows) + D.cps - 1) / D.cps; }      // workgroups (= slabs) per unit

// The chunks [c0, c1) of slice sl, with what row_chunk() needs beside them: it reads no descriptor field, because a kernel would
// reload those after every barrier of its chunk loop.  rereads_slab: something in a chunk adds to what the chunk's own backward
// stored (the GAIL gradient penalty), so not even a lone first chunk may stream
struct ChunkRange { int c0, c1, rc, rows, gs0; };      // gs0: the first chunk's GradStore
FRL_LAYOUT_FN ChunkRange chunk_range(const EngineDesc& D, int rows, int sl, bool rereads_slab = false) {
    const int nchunks = rowchunk_chunks(D, rows), c0 = sl * D.cps, c1 = c0 + D.cps;
    return ChunkRange{c0, c1 < nchunks ? c1 : nchunks, D.rc, rows, (D.cps > 1 || rereads_slab) ? GS_STORE : GS_STREAM};
}
// chunk ck of a range: how its gradients reach the slab, its first row, its valid rows (the last chunk of a unit may be ragged)
struct RowChunk { bool first; int gs, r0, nv; };
FRL_LAYOUT_FN RowChunk row_chunk(ChunkRange cr, int ck) {
    const bool first = (ck == cr.c0);
    const int r0 = ck * cr.rc, left = cr.rows - r0;
    return RowChunk{first, first ? cr.gs0 : GS_ADD, r0, cr.rc < left ? cr.rc : left};
}

// ------------------------------------------------------------------------------ (learner, agent, slice) -> floats / ints
FRL_LAYOUT_FN size_t unit_index(const EngineDesc& D, int p, int ag) { return (size_t)p * D.n_agents + ag; }
FRL_LAYOUT_FN size_t unit_slice_index(const EngineDesc& D, int p, int ag, int sl) { return unit_index(D, p, ag) * D.S + sl; }

// slab [P][S][learner_stride]: the agents' nets lie side by side inside a learner's stride, so a slice's slab serves all of them
FRL_LAYOUT_FN size_t slab_offset(const EngineDesc& D, int p, int sl, int net) { return ((size_t)p * D.S + sl) * D.learner_stride + D.net_off[net]; }
constexpr int kPartFloats = 4;      // part [P][n_agents][S][4]: {loss, entropy, -, -}
FRL_LAYOUT_FN size_t part_offset(const EngineDesc& D, int p, int ag, int sl) { return unit_slice_index(D, p, ag, sl) * kPartFloats; }
// idx [P][n_agents][batch_max]
FRL_LAYOUT_FN size_t idx_offset(const EngineDesc& D, int p, int ag, int r0) { return unit_index(D, p, ag) * D.batch_max + r0; }
// noise [P][n_agents][noise_sets][batch_max][act_max]
FRL_LAYOUT_FN size_t noise_set_floats(const EngineDesc& D) { return (size_t)D.batch_max * D.act_max; }
FRL_LAYOUT_FN size_t noise_offset(const EngineDesc& D, int p, int ag, int set, int r0) {
    return (unit_index(D, p, ag) * D.noise_sets + set) * noise_set_floats(D) + (size_t)r0 * D.act_max;
}
// act_spill [P][n_agents][S][2][rc][hidden + 4]: a chunk's h1 | h2 (adjacent in LDS, device/net.hpp: carve_lds) as one block
FRL_LAYOUT_FN int hidden_pitch(int hidden) { return hidden + 4; }
FRL_LAYOUT_FN int act_spill_pitch(const EngineDesc& D) { return 2 * D.rc * hidden_pitch(D.hidden); }
FRL_LAYOUT_FN size_t act_spill_offset(const EngineDesc& D, int p, int ag, int sl) { return unit_slice_index(D, p, ag, sl) * act_spill_pitch(D); }

// ------------------------------------------------------------------------------ CEM_GD3PG (kernels_cem_gd3pg.hip)
// The actor launch's units are (learner, actor) pairs of a single-agent engine: both actors of a learner share its idx and its part
// slots (the floats below), each has its net's region of the slice's slab and a spill block of its own.
constexpr int kCemActors = 2;
// a (learner, slice)'s part slot: the critic launch writes the first two floats, actor j of the actor launch float CEM_PART_ACTOR + j
enum CemPart : int { CEM_PART_CRITIC = 0, CEM_PART_C2 = 1, CEM_PART_ACTOR = 2 };      // squared TD errors | sum c^2 of the guided actor | -Q sums
static_assert(CEM_PART_ACTOR + kCemActors <= kPartFloats, "a part slot holds the critic's two sums and one per actor");
// act_spill [P][2 actors][S][2][rc][hidden + 4]
FRL_LAYOUT_FN size_t cem_spill_offset(const EngineDesc& D, int p, int actor, int sl) {
    return (((size_t)p * kCemActors + actor) * D.S + sl) * act_spill_pitch(D);
}
FRL_LAYOUT_FN size_t cem_spill_floats(const EngineDesc& D) { return cem_spill_offset(D, D.P, 0, 0); }
// the domain actor's output of row r0 .., parked by the critic launch for the guided actor's head delta: set 0 of the unit's noise block
// (no kernel of this algorithm draws noise)
FRL_LAYOUT_FN size_t cem_domain_offset(const EngineDesc& D, int p, int r0) { return noise_offset(D, p, 0, 0, r0); }

// ------------------------------------------------------------------------------ what the plan allocates
FRL_LAYOUT_FN size_t slab_floats(const EngineDesc& D) { return (size_t)D.P * D.S * D.learner_stride; }
FRL_LAYOUT_FN size_t part_floats(const EngineDesc& D) { return part_offset(D, D.P, 0, 0); }
FRL_LAYOUT_FN size_t act_spill_floats(const EngineDesc& D) { return act_spill_offset(D, D.P, 0, 0); }

}  // namespace frl
