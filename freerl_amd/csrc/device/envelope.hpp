// What the envelope kernels (kernels_envelope.hip, kernels_envelope_ddpg.hip) share: a row's preference vector written into the
// input columns of a net.
#pragma once
#include "net.hpp"

namespace frl {

// X[r][dst0 + k] = w[(r0 + r) / B][k] for r < nvalid, 0 for the rows past them
__device__ __forceinline__ void put_weights(lds_f X, int ldx, int rc, int nvalid, g_cf wts, int r0, int B, int RD, int dst0) {
    for (int e = threadIdx.x; e < rc * RD; e += kWG) {
        const int r = e / RD, k = e - r * RD;
        X[r * ldx + dst0 + k] = r < nvalid ? wts[(size_t)((r0 + r) / B) * RD + k] : 0.f;
    }
}

}  // namespace frl
