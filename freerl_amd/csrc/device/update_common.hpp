// Helpers shared by the row-chunk gradient kernels (kernels_dqn / _critic / _actor / _sacd / _reinforce / _envelope .hip):
// LDS carve from the engine descriptor, block id -> (unit, slice) on one XCD, the row chunks a workgroup walks.
// (The arithmetic of the policies and TD targets is in policy.hpp.)
#pragma once
#include "net.hpp"

namespace frl {

__device__ __forceinline__ Lds carve(const EngineDesc& D, float* smem) {
    return carve_lds(smem, D.rc, D.hidden, D.lds_kin_pad, D.lds_out_pad, D.lds_batch_pad, D.lds_act_pad, D.lds_hbufs);
}

// block id -> (unit, slice): the `ns` row chunks of unit u = learner*n_agents + agent sit on
// blocks {8*ns*g + x + 8s}, i.e. all on XCD x and adjacent in dispatch order.
struct UnitSlice { int unit, slice; };
__device__ __forceinline__ UnitSlice unit_slice(int ns) {
    const int group = 8 * ns, g = blockIdx.x / group, l = blockIdx.x - g * group;
    return UnitSlice{g * 8 + (l & 7), l >> 3};
}

// A workgroup owns `cps` consecutive row chunks of its unit (frl_create picks cps so that one round of workgroups fills
// the chip): chunk 0 stores its weight gradients in the workgroup's slab, the others add to them — one slab per
// workgroup instead of one per chunk for reduce_kernel to stream.
struct ChunkRange { int c0, c1; };
__device__ __forceinline__ ChunkRange chunk_range(const EngineDesc& D, int batch, int slab) {
    const int nchunks = (batch + D.rc - 1) / D.rc, c0 = slab * D.cps;
    return ChunkRange{c0, min(c0 + D.cps, nchunks)};
}

}  // namespace frl
