// The GAE recurrence as an affine suffix scan, shared by kernels_ppo.hip (ppo_gae_kernel, and gae_dense_kernel, which kernels_mappo /
// _mappo_mask / _mappo_state / _happo launch too) and kernels_gail_ppo.hip; the affine map itself also in float64 for ppo_gae_sb3_kernel
// and kernels_reinforce.hip's returns.
#pragma once
#include "net.hpp"

namespace frl {

// ---- GAE: A_t = delta_t + gamma*lambda*(1-adv_done_t)*A_{t+1}, reverse scan over the horizon.
// Affine maps m_t(x) = delta_t + g_t*x compose associatively; each thread folds a contiguous
// segment, a wave-shuffle suffix scan + 4 wave totals in LDS give every segment its incoming
// value, and the segment is replayed.  One workgroup per sequence.
template <class T> struct AffineT { T a, b; };
using Affine = AffineT<float>;
using AffineD = AffineT<double>;
template <class T>
__device__ __forceinline__ AffineT<T> compose(AffineT<T> f, AffineT<T> g) { return AffineT<T>{f.a * g.a, f.a * g.b + f.b}; }   // f(g(x))

__device__ __forceinline__ void gae_scan(g_cf delta, g_cf ring, int stride, int adv_done_col, int T, float c, g_f adv,
                                         lds_f lds) {
    const int t = threadIdx.x, L = (T + kWG - 1) / kWG;
    const int s0 = min(t * L, T), s1 = min(s0 + L, T);
    Affine f{1.f, 0.f};
    for (int i = s1 - 1; i >= s0; --i) {
        const float g = c * (1.f - ring[(size_t)i * stride + adv_done_col]);
        f = Affine{g * f.a, delta[i] + g * f.b};
    }
    // inclusive suffix scan inside the wave
    const int lane = t & 63, w = t >> 6;
    Affine s = f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Affine o{__shfl_down(s.a, off, 64), __shfl_down(s.b, off, 64)};
        if (lane + off < 64) s = compose(s, o);
    }
    if (lane == 0) { lds[2 * w] = s.a; lds[2 * w + 1] = s.b; }
    __syncthreads();
    float right = 0.f;                                    // A just right of this wave's last segment
    for (int ww = kWaves - 1; ww > w; --ww) right = lds[2 * ww] * right + lds[2 * ww + 1];
    const float mine = s.a * right + s.b;                 // A at the start of my segment
    float x = __shfl_down(mine, 1, 64);                   // A at the start of the next segment
    if (lane == 63) x = right;
    for (int i = s1 - 1; i >= s0; --i) {
        const float g = c * (1.f - ring[(size_t)i * stride + adv_done_col]);
        x = delta[i] + g * x;
        adv[i] = x;
    }
    __syncthreads();
}

}  // namespace frl
