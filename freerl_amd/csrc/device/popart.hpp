// PopArt DDPG's pieces of the row-chunk skeleton (kernels_popart.hip; DDPG_file/DDPG_simple_with_tricks.py:95-187): the net numbering, the
// learner's block in EngineDesc::popart, the batch-global statistics step that every reader derives for itself, and the upper layer's own
// optimiser step.  Every address comes from ../rowchunk_layout.h (tests/popart_plan_probe.cpp walks them against the plan's buffer sizes).
#pragma once
#include "adam.hpp"
#include "update_common.hpp"

namespace frl {

enum PopartNet : int { POP_ACTOR = 0, POP_CRITIC = 1 };
enum PopartOut : int { POP_OUT_CRITIC_LOSS = 0, POP_OUT_LOWER_NORM = 1, POP_OUT_UPPER_NORM = 2, POP_OUT_ACTOR_LOSS = 3, POP_OUT_ACTOR_NORM = 4,
                       POP_OUT_SIGMA = 5, POP_OUT_MU = 6, POP_OUT_ROWS = 7 };

__device__ __forceinline__ float* popart_head(const EngineDesc& D, int p) { return D.popart + popart_offset(D, p); }
__device__ __forceinline__ float* popart_part(const RowUnit& U) { return U.D.popart + popart_part_offset(U.D, U.p, U.sl); }
// the TD targets of rows r0 .., written by the target launch and read back by the critic launch
__device__ __forceinline__ g_f popart_y_rows(const RowUnit& U, int r0) { return as_global(U.D.popart + popart_y_offset(U.D, U.p, r0)); }

// The workgroup's sum of a double: the butterfly inside a wave on the two halves of the value, the four waves' sums through `red`
// (8 floats: four doubles as int pairs) and added in wave order, so every thread and every run holds the same bits
template <int OFF>
__device__ __forceinline__ double popart_lane_xor(double v) {
    const int lo = lane_xor<OFF>(__double2loint(v)), hi = lane_xor<OFF>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double popart_block_sum(double v, lds_f red) {
    v += popart_lane_xor<32>(v); v += popart_lane_xor<16>(v); v += popart_lane_xor<8>(v);
    v += popart_lane_xor<4>(v); v += popart_lane_xor<2>(v); v += popart_lane_xor<1>(v);
    FRL_LDS int* ri = (FRL_LDS int*)red;
    __syncthreads();                       // protect `red` from a previous use
    if (lane_id() == 0) {
        ri[2 * (threadIdx.x >> 6)] = __double2loint(v);
        ri[2 * (threadIdx.x >> 6) + 1] = __double2hiint(v);
    }
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kWG / 64; ++w) s += __hiloint2double(ri[2 * w + 1], ri[2 * w]);
    return s;
}

// art() and pop() (:128-139) of one learner's call, from the block's head as the previous call left it and the target launch's part
// slots added in slice order: mu', nu', sigma' and the popped W, b.  Every workgroup of the critic launch and the step kernel call this
// and hold the result in registers; the step kernel alone writes it back.  No contraction in here: the callers are different kernels
// and have to arrive at the same bits.
// guard: nu' - mu'^2 <= 0 (or NaN), where the reference's sqrt gives 0 or NaN and its division never recovers: sigma' = sigma
struct PopartStep { float W, b, sigma, mu, nu; bool guard; };
__device__ __forceinline__ PopartStep popart_next(const EngineDesc& D, int p, int ns, int B, float beta) {
#pragma clang fp contract(off)
    const float* hd = popart_head(D, p);
    double sy = 0.0, sy2 = 0.0;
    for (int k = 0; k < ns; ++k) {
        const double* pd = (const double*)(D.popart + popart_part_offset(D, p, k));
        sy += pd[POP_PART_SY / 2];
        sy2 += pd[POP_PART_SY2 / 2];
    }
    const float my = (float)(sy / (double)B), my2 = (float)(sy2 / (double)B);
    const float keep = (float)(1.0 - (double)beta);
    const float W = hd[POP_W], b = hd[POP_B], sigma = hd[POP_SIGMA], mu = hd[POP_MU], nu = hd[POP_NU];
    PopartStep n;
    n.mu = keep * mu + beta * my;
    n.nu = keep * nu + beta * my2;
    const float var = n.nu - n.mu * n.mu;
    n.guard = !(var > 0.f);
    n.sigma = n.guard ? sigma : sqrtf(var);
    const float rel = sigma / n.sigma;
    n.W = W * rel;
    n.b = b * rel + (mu - n.mu) / n.sigma;
    return n;
}

// PopArt.step()'s second half (:165-166) on the two parameters of the upper layer: clip_grad_norm_(0.5) over {dW, db} alone, then torch's
// Adam at step t with the moments in the block's head.  Returns the pre-clip norm; W and b are stepped in place
__device__ __forceinline__ float popart_upper_step(float* hd, float& W, float& b, float dW, float db, float lr, int t) {
    const float total = sqrtf(dW * dW + db * db);
    const AdamCoef c = adam_coef(total, 0.5f, t, lr, 0.9f, 0.999f, 1e-8f, 0.f, 0.f);
    float mW = hd[POP_MW], mb = hd[POP_MB], vW = hd[POP_VW], vb = hd[POP_VB];
    W = adam_exact1(W, dW * c.coef, mW, vW, c.w1, c.w2, c.beta2, c.bc2s, c.eps, c.step);
    b = adam_exact1(b, db * c.coef, mb, vb, c.w1, c.w2, c.beta2, c.bc2s, c.eps, c.step);
    hd[POP_MW] = mW; hd[POP_MB] = mb; hd[POP_VW] = vW; hd[POP_VB] = vb;
    return total;
}

}  // namespace frl
