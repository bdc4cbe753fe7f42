// What the two kernels of kernels_gail.hip share: the row gather of a call's expert and policy rows, torch's sigmoid / BCE arithmetic,
// and the pieces of the gradient penalty's second-order backward (GAIL_file/GAIL.py:88-98) that no first-order kernel has.
//
// The penalty c mean_e ||dl/dx||^2 of a piecewise-linear net, in closed form.  With m1, m2 the slopes (1 or `slope`) of a row's two
// hidden layers, u2 = m2 (.) w3, u1 = m1 (.) (W2^T u2), g = W1^T u1 = dl/dx, its gradient is a forward of the tangent t0 = 2 c g / E
// through the net without biases,
//     s1 = m1 (.) (W1 t0),  s2 = m2 (.) (W2 s1):      dW1 += u1 (x) t0,  dW2 += u2 (x) s1,  dw3 += s2,  biases: nothing
// (the second derivative of LeakyReLU / ReLU is zero, and autograd treats the slopes as constants).  The slopes are needed three
// times — forward, unit backward, tangent forward — while the activations they come from are overwritten by the first backward pass:
// they are kept as ONE BIT per unit (slope_pack), hidden / 32 words per row and layer in abuf / dabuf, instead of two more
// hidden-sized LDS buffers (which at hidden 256 would put a 32-row chunk past the 80 KB of two workgroups per CU).
#pragma once
#include "net.hpp"

namespace frl {

// slots of a workgroup's partial sums (EngineDesc::gail_part) and of a learner's results (EngineDesc::gail_out = frl_gail_args::out)
enum GailPart : int { GP_BCE_E = 0, GP_BCE_P = 1, GP_PEN = 2, GP_PROB_E = 3, GP_PROB_P = 4, GP_LOGIT_E = 5, GP_LOGIT_P = 6, GP_COUNT = 8 };
enum GailOut : int { GO_LOSS = 0, GO_PROB_E = 1, GO_PROB_P = 2, GO_WDIS = 3, GO_PEN = 4, GO_GNORM = 5 };

typedef FRL_LDS unsigned* lds_u;
typedef const FRL_LDS unsigned* lds_cu;

// torch.sigmoid in fp32: 1 for l >= 17, 0 for l <= -89 (exp overflows)
__device__ __forceinline__ float sigmoid_f(float l) { return 1.f / (1.f + expf(-l)); }
// F.binary_cross_entropy_with_logits of one element: softplus(-l) for target 1, softplus(l) for target 0
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// X[r][c] = row r0 + r of the call's E + N rows for c < ncols: expert ring row idx[j] (obs and action are adjacent in a record) for
// j < E, policy row j - E of the staged rows behind them, 0 past the call's rows
__device__ __forceinline__ void gail_gather(lds_f X, int ldx, int rc, int r0, int E, int NR, g_ci idx, g_cf ring, int stride, int src0,
                                            g_cf rows, int ncols) {
    for (int e = threadIdx.x; e < rc * ncols; e += kWG) {
        const int r = e / ncols, c = e - r * ncols, j = r0 + r;
        float v = 0.f;
        if (j < E) v = ring[(size_t)idx[j] * stride + src0 + c];
        else if (j < NR) v = rows[(size_t)(j - E) * ncols + c];
        X[r * ldx + c] = v;
    }
}

// bit k & 31 of word k >> 5 of row r: hidden unit k of that row was positive in the forward pass (slope 1)
__device__ __forceinline__ void slope_pack(lds_cf H, int ldh, int hidden, int rc, lds_u bits, int wpr) {
    const int nw = (hidden + 31) >> 5;
    for (int w = threadIdx.x; w < rc * nw; w += kWG) {
        const int r = w / nw, wi = w - r * nw;
        lds_cf src = H + r * ldh + 32 * wi;
        unsigned b = 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (32 * wi + 4 * q < hidden) {
                const f32x4 v = ld4(src + 4 * q);
                b |= (v.x > 0.f ? 1u : 0u) << (4 * q) | (v.y > 0.f ? 2u : 0u) << (4 * q) | (v.z > 0.f ? 4u : 0u) << (4 * q) | (v.w > 0.f ? 8u : 0u) << (4 * q);
            }
        bits[r * wpr + wi] = b;
    }
}
__device__ __forceinline__ bool slope_bit(lds_cu bits, int wpr, int r, int k) { return (bits[r * wpr + (k >> 5)] >> (k & 31)) & 1u; }

// Y[rc][n_pad] = m (.) (X[rc][k_pad] W^T): linear_fwd without the bias, each unit's slope from its packed bit
__device__ __forceinline__ void tangent_fwd(const LayerDesc& L, g_cf theta, lds_cf X, int ldx, lds_f Y, int ldy, int rc, lds_cu bits,
                                            int wpr, float slope) {
    g_cf W = theta + L.w_off;
    const int kpad = L.k_pad, npad = L.n_pad;
    auto finish = [&](int r, int c4, f32x4 v) {
        const unsigned b = bits[r * wpr + (c4 >> 5)] >> (c4 & 31);          // c4 is a multiple of 4: its four bits share a word
        v.x *= (b & 1u) ? 1.f : slope; v.y *= (b & 2u) ? 1.f : slope; v.z *= (b & 4u) ? 1.f : slope; v.w *= (b & 8u) ? 1.f : slope;
        st4(Y + r * ldy + c4, v);
    };
    if (npad % 64 == 0) {
        for_il_blocks(rc / 16, npad / 64, [&](auto bm, int mt0, int g) {
            constexpr int BM = decltype(bm)::value;
            f32x4 acc[BM][4];
            acc_zero(acc);
            mma_w_any<BM, 4, W_IL>(acc, X, ldx, mt0 * 16, W, npad, g * 64, kpad);
            tile_epilogue<BM, 4, W_IL>(acc, mt0 * 16, g * 64, [&](int r, int c4, f32x4 v, int) { finish(r, c4, v); });
        });
    } else {
        for_tile_blocks(rc / 16, npad / 16, [&](auto bm, auto bn, int mt0, int nt0) {
            constexpr int BM = decltype(bm)::value, BN = decltype(bn)::value;
            f32x4 acc[BM][BN];
            acc_zero(acc);
            mma_w_any<BM, BN, W_ROWS>(acc, X, ldx, mt0 * 16, W, npad, nt0 * 16, kpad);
            tile_epilogue<BM, BN, W_ROWS>(acc, mt0 * 16, nt0 * 16, [&](int r, int c4, f32x4 v, int) { finish(r, c4, v); });
        });
    }
}

// G.w3[k] += sum_r s2[r][k] for a head the BCE pass took through head_bwd: the same owner of unit k (two lanes of one wave, half of
// the rows each, the lower one stores), so the running sum it reads back is its own store
__device__ __forceinline__ void head_tangent_dw(const LayerDesc& LH, g_f G, lds_cf H, int ldh, int rc) {
    const int l = lane_id(), half = l >> 5, k = (threadIdx.x >> 6) * 32 + (l & 31);
    const int hr = rc / 2, r_lo = half * hr;
    if (k < LH.k_pad) {
        g_f g = G + LH.w_off + k * 16;
        const float old = half == 0 ? *g : 0.f;
        float p[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = r_lo; r < r_lo + hr; r += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] += H[(r + j) * ldh + k];
        }
        float s = (p[0] + p[1]) + (p[2] + p[3]);
        s += lane_xor<32>(s);
        if (half == 0) *g = old + s;
    }
}

}  // namespace frl
