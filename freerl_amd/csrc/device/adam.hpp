// The optimiser arithmetic every learner update shares: torch's clip_grad_norm_ coefficient, single-tensor Adam with its bias
// corrections in fp64 (torch computes `beta ** step` in Python floats), and SAC's temperature step.  The loops that stream the
// parameters stay with their kernels; only the arithmetic is here.
#pragma once
#include "../frl_desc.h"
#include "tile.hpp"

namespace frl {

// beta^t in double by repeated squaring (torch computes `beta ** step` in Python floats)
__device__ __forceinline__ double powi_d(double b, int t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

// (no flags in here: the register-chained update runs inside MFMA chains, where a branch would cut the scheduling region — the
// soft target update is a template argument of its functions, weight decay is applied unconditionally: g + 0 * theta = g)
struct AdamCoef { float coef, step, bc2s, inv_bc2s, w1, w2, beta2, eps, wd, tk, tau; };

// clip coefficient (clip_norm > 0: min(clip / (total + 1e-6), 1)) and the coefficients of Adam step t; tk / tau: soft target update
__device__ __forceinline__ AdamCoef adam_coef(float total, float clip_norm, int t, float lr, float beta1, float beta2, float eps,
                                              float wd, float tau) {
    AdamCoef c;
    c.coef = clip_norm > 0.f ? fminf(clip_norm / (total + 1e-6f), 1.f) : 1.f;
    const double bc1 = 1.0 - powi_d((double)beta1, t), bc2 = 1.0 - powi_d((double)beta2, t);
    c.step = (float)((double)lr / bc1); c.bc2s = (float)sqrt(bc2); c.inv_bc2s = 1.f / c.bc2s;
    c.w1 = 1.f - beta1; c.w2 = 1.f - beta2; c.beta2 = beta2; c.eps = eps; c.wd = wd;
    c.tk = 1.f - tau; c.tau = tau;
    return c;
}

// torch's Adam on one element (g: clip coefficient and weight decay already applied), correctly rounded sqrt and division: the
// row-chunk update (kernels_update.hip), solo / solow (solo.hpp, solo_wide.hpp), kernels_dqn2.hip and adam_net (PPO)
__device__ __forceinline__ float adam_exact1(float th, float g, float& m, float& v, float w1, float w2, float b2, float bc2s, float eps,
                                             float step) {
    m = m + (g - m) * w1;
    v = v * b2 + (w2 * g) * g;
    return th - step * (m / (sqrtf(v) / bc2s + eps));
}
__device__ __forceinline__ f32x4 adam_exact4(f32x4 th, f32x4 g, f32x4& m, f32x4& v, float w1, float w2, float b2, float bc2s, float eps,
                                             float step) {
    m = m + (g - m) * w1;
    v = v * b2 + (w2 * g) * g;
    f32x4 denom;
#pragma unroll
    for (int r = 0; r < 4; ++r) denom[r] = sqrtf(v[r]) / bc2s + eps;
    return th - step * (m / denom);
}

// The same step with the hardware's 1-ulp sqrt and reciprocal: kernels_critic2 / _actor2 (chain_net.hpp), the K-sliced and
// x-stationary kernels (chain_wide.hpp's adam_stream) and kernels_ppo2.hip.  The moments are the exact fp32 fma chains above;
// only step * m / (sqrt(v) / sqrt(bc2) + eps) leaves the correctly rounded sequences (3 x ~10 VALU instructions per element, 88
// elements per lane and step: the difference between a 28 k and an 8 k cycle Adam phase).  Its relative error (<= ~3 ulp of the
// UPDATE, which is itself ~lr times smaller than the parameter) is below the rounding of the subtraction that applies it.
__device__ __forceinline__ float adam_elem(float th, float g, float& m, float& v, float w1, float w2, float b2, float inv_bc2s,
                                           float eps, float step) {
    m = m + (g - m) * w1;
    v = v * b2 + (w2 * g) * g;
    const float denom = __builtin_amdgcn_sqrtf(v) * inv_bc2s + eps;
    return th - step * (m * __builtin_amdgcn_rcpf(denom));
}

// SAC.py:251, the actor loss stat: (alpha log pi - Q).mean() (qtot: both critics' Q summed); -Q.mean() otherwise
__device__ __forceinline__ float actor_loss_stat(bool sac, float qtot, float lptot, float alpha, float invB) {
    return sac ? (-(qtot * 0.5f) + alpha * lptot) * invB : -qtot * invB;
}

// SAC's alpha step on the batch's entropy (SAC.py:154-169,257-260): Adam on log_alpha with torch's default eps 1e-8 (not the nets'
// adam_eps) and its own step count *count.  al = {log_alpha, m, v, alpha}, alpha = al[3] before the step; st = the unit's stats row.
__device__ __forceinline__ void sac_alpha_step_at(float* al, float* st, int* count, float alpha, float ent_mean, float target_entropy,
                                                  float beta1, float beta2, float alpha_lr) {
    const float mean_term = ent_mean - target_entropy;
    const float gl = alpha * mean_term;                                // d alpha_loss / d log_alpha
    const int ta = *count + 1;
    float mi = al[1], vi = al[2];
    mi = mi + (gl - mi) * (1.f - beta1);
    vi = vi * beta2 + ((1.f - beta2) * gl) * gl;
    const double b1 = 1.0 - powi_d((double)beta1, ta), b2 = 1.0 - powi_d((double)beta2, ta);
    const float denom = sqrtf(vi) / (float)sqrt(b2) + 1e-8f;
    al[0] = al[0] - (float)((double)alpha_lr / b1) * (mi / denom);
    al[1] = mi;
    al[2] = vi;
    al[3] = expf(al[0]);
    *count = ta;
    st[ST_ALPHA_LOSS] = alpha * mean_term;
    st[ST_ALPHA] = al[3];
    st[ST_ENTROPY] = ent_mean;
}
// ... of a single-agent SAC engine: the learner's one alpha block, its step count in steps[kMaxNets]
__device__ __forceinline__ void sac_alpha_step(float* al, float* st, int* steps, float alpha, float ent_mean, float target_entropy,
                                               float beta1, float beta2, float alpha_lr) {
    sac_alpha_step_at(al, st, steps + kMaxNets, alpha, ent_mean, target_entropy, beta1, beta2, alpha_lr);
}
// MASAC (MASAC.py:124-139,271-273): agent ag's own alpha block of EngineDesc::alpha [P][n][4], its step count behind the nets' counters,
// target entropy -act_dim[ag]
__device__ __forceinline__ void masac_alpha_step(const EngineDesc& D, int p, int ag, float* st, float ent_mean, float beta1, float beta2, float alpha_lr) {
    float* al = D.alpha + ((size_t)p * D.n_agents + ag) * 4;
    int* count = D.steps + (size_t)D.P * (kMaxNets + 1) + (size_t)p * D.n_agents + ag;
    sac_alpha_step_at(al, st, count, al[3], ent_mean, -(float)D.rec.act_dim[ag], beta1, beta2, alpha_lr);
}

}  // namespace frl
