// The per-element arithmetic of the reference's continuous policies and TD targets, shared by every kernel family that runs it:
// the log_std clamp and its gradient gate, the Normal log-prob term and the tanh correction, SAC's tanh-Gaussian sample, TD3's
// target-policy smoothing, the TD target and the TD loss, the actor's head deltas through tanh.  Scalar functions on float only:
// the loops, the lane mappings, LDS and the reductions stay with their kernels.  Arguments are evaluated at the call: an operand
// that is a memory read of one algorithm only stays under that algorithm's branch at the call site.
#pragma once
#include "../frl_desc.h"

namespace frl {

constexpr float kLogSqrt2Pi = 0.91893853320467274178f;
constexpr float kLog2 = 0.69314718055994530942f;
constexpr float kLogStdMin = -20.f, kLogStdMax = 2.f;

__device__ __forceinline__ float softplus_t(float x) {     // F.softplus (beta 1, threshold 20)
    return x > 20.f ? x : log1pf(expf(x));
}

// TD loss of one row's error e: value and d/de (before the 1/B of the mean).  MSE: e^2, 2e.  Huber (MAPPO.py:273-276).
// Every critic / Q kernel: kernels_critic / _critic2 / _criticw / _criticx / _solo / _solow / _dqn / _dqn2 / _sacd.
__device__ __forceinline__ void td_loss_row(const LearnArgs& a, float e, float& loss, float& grad) {
    if (a.huber) {
        const float d = a.huber_delta, ae = fabsf(e);
        if (ae <= d) { loss = e * e * 0.5f; grad = e; }
        else { loss = d * (ae - d * 0.5f); grad = e > 0.f ? d : -d; }
    } else {
        loss = e * e; grad = 2.f * e;
    }
}

// log_std = clamp(log_std, -20, 2) (SAC.py:76, PPO_with_tricks.py:102): every kernel that reads a log_std — the SAC
// sample and log_std gradient below, kernels_ppo2, act_common.hpp; clamp_range is the same over a given range: onpolicy.hpp's Normal head
// (kernels_ppo and mappo_steps with kLogStdMin / kLogStdMax, kernels_gail_ppo with the engine's)
__device__ __forceinline__ float clamp_range(float raw, float lo, float hi) { return fminf(fmaxf(raw, lo), hi); }
__device__ __forceinline__ float clamp_log_std(float raw) { return clamp_range(raw, kLogStdMin, kLogStdMax); }
// torch.clamp passes no gradient outside its bounds: the log_std gradient of every SAC actor kernel (kernels_actor / _actor2 /
// _actorw / _actorx / _solo / _solow) and of kernels_ppo2; the ranged form gates the streaming on-policy kernels' log_std
__device__ __forceinline__ bool log_std_grad_open(float raw, float lo, float hi) { return raw >= lo && raw <= hi; }      // (the CLOSED range)
__device__ __forceinline__ bool log_std_grad_open(float raw) { return log_std_grad_open(raw, kLogStdMin, kLogStdMax); }

// Normal(mean, sd).log_prob(x), d = x - mean, ls = log(sd) (SAC.py:86, torch.distributions.Normal): sac_sample below and its
// written-out forms (kernels_criticw / _criticx / _actorx), onpolicy.hpp's normal_row_logp and kernels_ppo2 (the stored action
// against the current mean), act_common.hpp and kernels_gail_ppo (ACT_PPO_SAMPLE)
__device__ __forceinline__ float normal_logp(float d, float sd, float ls) { return -(d * d) / (2.f * sd * sd) - ls - kLogSqrt2Pi; }
// log(1 - tanh(u)^2) in its stable form 2 (log 2 - u - softplus(-2u)) (SAC.py:87): sac_sample, kernels_criticw / _criticx / _actorx
__device__ __forceinline__ float tanh_logp_correction(float u) { return 2.f * (kLog2 - u - softplus_t(-2.f * u)); }

// SAC.py:70-97, one action component: u = mean + exp(clamp(log_std)) eps; lp += log N(u) - log(1 - tanh(u)^2); returns tanh(u).
// On the target actor (SAC.py:227) in kernels_critic / _critic2 / _solo / _solow, on the online actor (SAC.py:244) in
// kernels_actor / _actor2 / _actorw / _solo / _solow.  (kernels_criticw / _criticx / _actorx write these steps out from the pieces
// above: there eps is a global read that, as an argument, would be loaded ahead of expf, which moves their spill counts.)
__device__ __forceinline__ float sac_sample(float mean, float raw_log_std, float eps, float& lp) {
    const float ls = clamp_log_std(raw_log_std), sd = expf(ls);
    const float u = mean + sd * eps, du = u - mean;
    lp += normal_logp(du, sd, ls);
    lp -= tanh_logp_correction(u);
    return tanhf(u);
}

// TD3.py:196-198 / MATD3_simple.py:204-205, one component: v = tanh(actor_target(s')), nz ~ N(0, 1); returns
// clip(v max_action + clip(noise, -c, c), -max_action, max_action) / max_action.  The target pass of kernels_critic / _critic2 /
// _criticw / _criticx / _solo / _solow.
__device__ __forceinline__ float td3_smooth(const LearnArgs& a, float v, float nz) {
    float n1 = a.policy_noise_scale * (nz * a.policy_noise);
    n1 = fminf(fmaxf(n1, -a.noise_clip), a.noise_clip);
    return fminf(fmaxf(v * a.max_action + n1, -a.max_action), a.max_action) / a.max_action;
}

// y = r + gamma (1 - d) (min Q' - alpha log pi') (SAC.py:232-235) and y = r + gamma Q' (1 - d) (DDPG_simple.py:146, TD3.py:209,
// MADDPG_simple.py:173, MATD3_simple.py:235): the target pass of kernels_critic / _critic2 / _criticw / _criticx / _solo / _solow
__device__ __forceinline__ float td_target_sac(float rew, float done, float gamma, float q, float alpha, float lp) {
    return rew + gamma * (1.f - done) * (q + alpha * (-lp));
}
__device__ __forceinline__ float td_target(float rew, float done, float gamma, float q) { return rew + gamma * q * (1.f - done); }

// The actor's head delta through a = tanh(.): dq = d loss / d a (DDPG_simple.py:153, TD3.py:227); SAC adds alpha log pi's
// 2a (alpha / B) (SAC.py:87,251), and d loss / d log_std of one row is the mean's delta times exp(log_std) eps, minus alpha / B
// (SAC.py:83,86).  The last pass of kernels_actor / _actor2 / _actorw / _actorx / _solo / _solow (kernels_actorx writes the
// log_std term out, for the same read of eps).
__device__ __forceinline__ float tanh_delta(float dq, float av) { return dq * (1.f - av * av); }
__device__ __forceinline__ float sac_mean_delta(float dq, float av, float alpha, float invB) {
    return dq * (1.f - av * av) + (alpha * invB) * (2.f * av);
}
__device__ __forceinline__ float sac_log_std_grad(float d, float raw_log_std, float eps, float alpha, float invB) {
    const float ls = clamp_log_std(raw_log_std);
    return d * expf(ls) * eps - alpha * invB;
}

// The per-row log_std forms (MASAC.py:37-68: log_std is a head column beside the mean, clamped per row) of an actor loss whose Q
// term and entropy term come from TWO draws of the same forward (MASAC.py:254-261): a1 = tanh(mean + sd eps1) went into Q, dq = d loss /
// d a1; the entropy is -log pi of u2 = mean + sd eps2, weighted alpha / B.  d log pi / d u2 = 2 tanh(u2) (the Normal term's own
// dependence on the mean cancels under rsample), d log pi / d log_std = 2 tanh(u2) sd eps2 - 1.  kernels_masac.hip.
__device__ __forceinline__ float sac2_mean_delta(float dq, float a1, float t2, float alpha, float invB) {
    return dq * (1.f - a1 * a1) + (alpha * invB) * (2.f * t2);
}
__device__ __forceinline__ float sac2_log_std_delta(float dq, float a1, float t2, float raw_log_std, float eps1, float eps2, float alpha, float invB) {
    if (!log_std_grad_open(raw_log_std)) return 0.f;      // torch.clamp passes no gradient outside its (closed) bounds
    const float sd = expf(clamp_log_std(raw_log_std));
    return dq * (1.f - a1 * a1) * (sd * eps1) + (alpha * invB) * ((2.f * t2) * (sd * eps2) - 1.f);
}

}  // namespace frl
