// MASAC (MAAC_file/MASAC.py) on the row-chunk primitives of net.hpp: the one buffer its actor stage needs behind the common carve.
// The actor's head is [mean | log_std], 2 A columns of outb; the updating agent's head row must survive the two critic passes that
// reuse outb (the head delta is formed from it afterwards), so it is parked in `head`: EngineDesc::lds_row_extra floats per row.
#pragma once
#include "net.hpp"

namespace frl {

struct MasacLds {
    lds_f head; int sp;      // [rc][sp] the updating actor's [mean | raw log_std] of a row, sp = masac_row_extra(act_max)
};

// must mirror engine_plan.hpp: lds_bytes_for() with lds_row_extra = masac_row_extra(act_max)
__device__ __forceinline__ MasacLds carve_masac(const EngineDesc& D, const Lds& S, float* smem) {
    MasacLds M;
    M.sp = D.lds_row_extra;
    M.head = (lds_f)smem + D.rc * (S.xp + D.lds_hbufs * S.hp + S.op + 2 * S.ap) + D.lds_batch_pad + 8;
    return M;
}

}  // namespace frl
