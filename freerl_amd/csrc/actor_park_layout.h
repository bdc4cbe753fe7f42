// Where the eight-wave chained actor stage (kernels_actor2.hip, ac_actor_v2_body<8, 1, true>) parks pass A's second hidden layer h2
// for pass C: one 16-byte slot per (learner, pass-C chunk, tile, wave, lane), laid out [learner][chunk][tile][wave][lane] so that one
// wave instruction covers 1 KB contiguously.  The tiles are h2's eight feature tiles.  A lane reads back only the slots it wrote
// itself, within the launch.  Plain C++17 (no HIP): the kernel, the engine plan's count (engine_plan.hpp) and
// tests/actor_park_probe.cpp read the same functions, so the allocated size and the largest touched offset are one formula.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define FRL_PARK_FN __host__ __device__ __forceinline__
#else
#define FRL_PARK_FN inline
#endif

namespace frl {

constexpr int kParkRows = 256;                                  // rows of a learner's batch the carve provides (device/chain_net.hpp: kChainBatch)
constexpr int kParkWaves = 8, kParkLanes = 64;                  // the eight-wave workgroup
constexpr int kParkChunkRows = 16 * kParkWaves;                 // rows of a pass-C chunk: a 16-row tile per wave
constexpr int kParkChunks = kParkRows / kParkChunkRows;
constexpr int kParkTiles = 8;                                   // feature tiles of h2 per (chunk, wave)
constexpr int kParkSlotFloats = 4;                              // one f32x4 per lane

// slot number (in f32x4 units) of (learner p, chunk c, tile, wave w, lane l)
FRL_PARK_FN size_t actor_park_slot(int p, int c, int tile, int w, int l) {
    return ((((size_t)p * kParkChunks + c) * kParkTiles + tile) * kParkWaves + w) * kParkLanes + l;
}
// slots between the same lane's consecutive tiles
constexpr int kParkTileStride = kParkWaves * kParkLanes;
// floats the plan allocates for P learners: 128 KiB per learner
FRL_PARK_FN size_t actor_park_floats(int P) { return actor_park_slot(P, 0, 0, 0, 0) * kParkSlotFloats; }

}  // namespace frl
