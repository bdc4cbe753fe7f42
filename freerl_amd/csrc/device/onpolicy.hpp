// The head arithmetic of the reference's on-policy (PPO-family) updates, shared by every kernel family that runs it: kernels_ppo /
// _ppo2 (PPO_file/PPO_with_tricks.py), kernels_gail_ppo (GAIL_file/PPO2.py), device/mappo.hpp's mappo_steps (MAPPO_file/MAPPO.py,
// IPPO.py, HAPPO.py and the two masked variants), kernels_happo, kernels_reinforce and act_common.hpp's categorical draw.  The rules
// are device/policy.hpp's: the small pieces are scalar functions on float, evaluated in the order of the call site; the LDS block
// loops take the Lds carve and plain arguments.  What is a family's own stays with it: the step loops, their optimisers, the one
// mlp_bwd / mappo_bwd call site per net role (the helpers here run before it and never wrap it), and the ORDER in which a family
// scales the surrogate's open advantage — (open * (-1/m)) * ratio in PPO and GAIL, (-sum open * ratio) / (m n) in MAPPO, the row
// factor first in HAPPO.
#pragma once
#include "net.hpp"

namespace frl {

constexpr float kProbEps = 1.1920929e-07f;                         // torch.finfo(float32).eps: Categorical(probs=)'s clamp
constexpr float kHalfLog2PiPlusHalf = 1.41893853320467274178f;     // 0.5 + 0.5 log(2 pi): Normal.entropy() - log_std

// ---- clipped surrogate of one (ratio, advantage) pair (PPO_with_tricks.py:324-346, PPO2.py:282-292, MAPPO.py:410-412): adds
// -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A) to `loss`, returns the advantage where the gradient is open (s1 <= s2), else 0
__device__ __forceinline__ float surrogate_term(float ratio, float A, float clip, float& loss) {
    const float s1 = ratio * A, s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * A;
    loss += -fminf(s1, s2);
    return s1 <= s2 ? A : 0.f;
}

// ---- Normal head: mean = tanh(head row), std = exp(clamp(log_std, lo, hi)) with log_std a parameter vector behind the net.  The
// range is policy.hpp's kLogStdMin / kLogStdMax (PPO_with_tricks.py:102, which MAPPO.py's actors follow) or the engine's (PPO2.py:38);
// the clamp and its gradient gate are policy.hpp's clamp_range and log_std_grad_open(raw, lo, hi).

// Normal.log_prob(action) summed over the A action columns of one row (PPO_with_tricks.py:324-346, PPO2.py:250,282, MAPPO.py:399-412): ONE
// definition for the update steps, GAIL's old-log-prob pass and HAPPO's two horizon passes, so that a ratio cannot drift from its parts
__device__ __forceinline__ float normal_row_logp(g_cf act, lds_cf mean, g_cf log_std_raw, int A, float lo, float hi) {
    float lp = 0.f;
    for (int c = 0; c < A; ++c) {
        const float ls = clamp_range(log_std_raw[c], lo, hi);
        lp += normal_logp(act[c] - mean[c], expf(ls), ls);
    }
    return lp;
}

// 1 - m^2, the derivative of m = tanh(z), with the product rounded on its own.  Contraction is switched off here because it is the
// one place of this header where the compiler's choice moved with the surrounding code: every family's build paired m * m with its
// neighbour dm * dm in one packed multiply and subtracted afterwards, and a fused multiply-add gives other bits.
__device__ __forceinline__ float one_minus_sq(float m) {
#pragma clang fp contract(off)
    return 1.f - m * m;
}

// The head's deltas of one chunk once every row's coef = d loss / d (sum_c log-prob) stands in dabuf[r * ap]: outb <- the mean's
// delta through tanh (zero in invalid rows and pad columns), abuf <- the log_std delta per row, and thread c < A adds column c's sum
// over the chunk to `gls` (PPO_with_tricks.py:324-346, PPO2.py:282-292, MAPPO.py:399-412).  The stored action of chunk row r is
// ring[idx[r] * stride + act_col ..].  Starts and ends with a barrier.
__device__ __forceinline__ void normal_head_delta(const Lds& S, int nv, int A, int npad, g_ci idx, g_cf ring, int stride, int act_col,
                                                  g_cf log_std_raw, float lo, float hi, float& gls) {
    __syncthreads();
    for (int e = threadIdx.x; e < S.rc * npad; e += kWG) {
        const int r = e / npad, c = e - r * npad;
        float d = 0.f, dl = 0.f;
        if (r < nv && c < A) {
            const float coef = S.dabuf[r * S.ap];
            const float mean = S.outb[r * S.op + c];
            const float var = expf(2.f * clamp_range(log_std_raw[c], lo, hi));
            const float dm = ring[(size_t)idx[r] * stride + act_col + c] - mean;
            d = coef * dm / var * one_minus_sq(mean);         // through mean = tanh(z)
            dl = coef * (dm * dm / var - 1.f);
        }
        S.outb[r * S.op + c] = d;
        if (c < A) S.abuf[r * S.ap + c] = dl;
    }
    __syncthreads();
    if ((int)threadIdx.x < A)
        for (int r = 0; r < S.rc; ++r) gls += S.abuf[r * S.ap + threadIdx.x];
}

// ---- Categorical head.  The three unmasked forms of the reference produce different bits and stay apart:
//   CAT_PROBS     Categorical(probs = softmax(z)) (PPO_with_tricks.py:333-336, MAPPO.py:399-412, HAPPO.py:382-391, REINFORCE.py:82-85):
//                 p = exp(z - mx) / sum, renormalised by its own sum, log-prob = log(clamp(p / psum, eps, 1 - eps))
//   CAT_LOGITS_Q  PPO with EngineDesc::cat_logits (PPO_file/PPO.py:176,257): p as above, log-prob = (z - mx) - lse
//   CAT_LOGITS_E  Categorical(logits = z) (PPO2.py:247,279): log-prob = (z - mx) - lse, p = exp(log-prob)
enum CatKind { CAT_PROBS = 0, CAT_LOGITS_Q = 1, CAT_LOGITS_E = 2 };
struct CatRow {
    float mx, sum, psum, lse;
    int kind;
    __device__ __forceinline__ float prob(float z) const { return expf(z - mx) / sum; }                 // softmax entry
    __device__ __forceinline__ float logit(float z) const { return (z - mx) - lse; }                    // log-softmax entry
    __device__ __forceinline__ float clamped(float p) const { return fminf(fmaxf(p / psum, kProbEps), 1.f - kProbEps); }
    __device__ __forceinline__ float logp(float p) const { return logf(clamped(p)); }                  // CAT_PROBS' log-prob
    // column z's probability and log-prob as the row's form has them
    __device__ __forceinline__ void col(float z, float& p, float& lg) const {
        if (kind == CAT_LOGITS_E) { lg = logit(z); p = expf(lg); }
        else { p = prob(z); lg = kind == CAT_LOGITS_Q ? logit(z) : logp(p); }
    }
    __device__ __forceinline__ float entropy(lds_cf z, int A) const {                                   // -sum_c p_c log-prob_c
        float h = 0.f;
        for (int c = 0; c < A; ++c) { float p, lg; col(z[c], p, lg); h -= lg * p; }
        return h;
    }
    __device__ __forceinline__ float logp_at(lds_cf z, int A, int a) const {                            // 0 for an index outside [0, A)
        float lp = 0.f;
        for (int c = 0; c < A; ++c)
            if (c == a) { float p; col(z[c], p, lp); }
        return lp;
    }
    // the head delta of column c: coef (1[c = a] - p_c) + ent_m p_c (log-prob_c + H)
    __device__ __forceinline__ float delta(float zc, int c, int a, float coef, float ent_m, float H) const {
        float p, lg;
        col(zc, p, lg);
        return coef * ((c == a ? 1.f : 0.f) - p) + ent_m * p * (lg + H);
    }
};
// the softmax part alone: psum is left 0 for a caller that walks the probabilities anyway and adds them up, in class order, itself
// (act_common.hpp's draw, REINFORCE's in-place row)
__device__ __forceinline__ CatRow cat_softmax(lds_cf z, int A, int kind = CAT_PROBS) {
    CatRow q;
    q.kind = kind;
    q.mx = z[0];
    for (int c = 1; c < A; ++c) q.mx = fmaxf(q.mx, z[c]);
    q.sum = 0.f;
    for (int c = 0; c < A; ++c) q.sum += expf(z[c] - q.mx);
    q.psum = 0.f;
    q.lse = logf(q.sum);
    return q;
}
// (a form that reads no psum or lse leaves their loops dead: `kind` is a constant at every call site but PPO's)
__device__ __forceinline__ CatRow cat_row(lds_cf z, int A, int kind = CAT_PROBS) {
    CatRow q = cat_softmax(z, A, kind);
    for (int c = 0; c < A; ++c) q.psum += q.prob(z[c]);
    return q;
}

// CategoricalMasked (MAPPO_for_mask_action.py:191-215) of one row: logits' = where(mask, z, -1e8), Categorical(logits = logits').  The
// normalised logit is l = logits' - (max + log sum exp(logits' - max)), in torch's order: in a row whose mask is all closed the
// bracket rounds back to -1e8 and every l is exactly 0 (p = 1 / A, log-prob 0), where (z - max) - log sum would give -log A.
// p = softmax(l); a closed column has p = 0 exactly next to an open one.  `mask` is the row's block in its ring record: nonzero = open.
constexpr float kMaskedLogit = -1e8f;
struct MaskedCatRow {
    g_cf mask;
    float lse, lmx, sum;
    __device__ __forceinline__ bool open(int c) const { return mask[c] != 0.f; }
    __device__ __forceinline__ float logit(float z, int c) const { return (open(c) ? z : kMaskedLogit) - lse; }      // l_c
    __device__ __forceinline__ float prob(float l) const { return expf(l - lmx) / sum; }
    // entropy(): -sum over the open columns of p_c l_c
    __device__ __forceinline__ float entropy(lds_cf z, int A) const {
        float h = 0.f;
        for (int c = 0; c < A; ++c)
            if (open(c)) { const float l = logit(z[c], c); h -= prob(l) * l; }
        return h;
    }
    __device__ __forceinline__ float logp_at(lds_cf z, int A, int a) const {
        float lp = 0.f;
        for (int c = 0; c < A; ++c)
            if (c == a) lp = logit(z[c], c);
        return lp;
    }
    // the head delta of column c: CatRow's where open, 0 where closed (torch.where passes no gradient)
    __device__ __forceinline__ float delta(float zc, int c, int a, float coef, float ent_m, float H) const {
        if (!open(c)) return 0.f;
        const float l = logit(zc, c), pc = prob(l);
        return coef * ((c == a ? 1.f : 0.f) - pc) + ent_m * pc * (l + H);
    }
};
__device__ __forceinline__ MaskedCatRow masked_cat_row(lds_cf z, g_cf mask, int A) {
    MaskedCatRow q;
    q.mask = mask;
    auto sub = [&](int c) { return mask[c] != 0.f ? z[c] : kMaskedLogit; };
    float mx = sub(0);
    for (int c = 1; c < A; ++c) mx = fmaxf(mx, sub(c));
    float s = 0.f;
    for (int c = 0; c < A; ++c) s += expf(sub(c) - mx);
    q.lse = mx + logf(s);
    q.lmx = sub(0) - q.lse;
    for (int c = 1; c < A; ++c) q.lmx = fmaxf(q.lmx, sub(c) - q.lse);
    q.sum = 0.f;
    for (int c = 0; c < A; ++c) q.sum += expf((sub(c) - q.lse) - q.lmx);
    return q;
}

// The categorical head's deltas of one chunk, one thread per row: for chunk row r < nv, q = dist(r, z) is the row's distribution
// (CatRow or MaskedCatRow) and a = action(r) the stored index; coef(r, log-prob of a, H) folds the row into the caller's loss sums and
// returns d loss / d log-prob; the row's delta is staged in abuf (outb is still being read by the row) and copied to outb, zero in
// invalid rows and pad columns.  Ends with a barrier.
template <class Dist, class Action, class Coef>
__device__ __forceinline__ void cat_head_delta(const Lds& S, int nv, int A, int npad, float ent_m, Dist dist, Action action, Coef coef) {
    if ((int)threadIdx.x < S.rc) {
        const int r = threadIdx.x;
        lds_cf z = S.outb + r * S.op;
        if (r < nv) {
            const auto q = dist(r, z);
            const int a = action(r);
            const float H = q.entropy(z, A);
            const float cf = coef(r, q.logp_at(z, A, a), H);
            for (int c = 0; c < npad; ++c) S.abuf[r * S.ap + c] = c < A ? q.delta(z[c], c, a, cf, ent_m, H) : 0.f;
        } else {
            for (int c = 0; c < npad; ++c) S.abuf[r * S.ap + c] = 0.f;
        }
        for (int c = 0; c < npad; ++c) S.outb[r * S.op + c] = S.abuf[r * S.ap + c];
    }
    __syncthreads();
}

// ---- critic regression of one chunk (PPO_with_tricks.py:349-351, PPO2.py:295-298): column 0 of valid row r gets scale * 2 diff / m
// with diff = V - target[idx[r]], every other entry of outb 0, `loss` += diff^2.  Ends with a barrier.
__device__ __forceinline__ void critic_delta_rows(const Lds& S, int nv, int npad, g_ci idx, g_cf target, float scale, float invm, float& loss) {
    for (int e = threadIdx.x; e < S.rc * npad; e += kWG) {
        const int r = e / npad, c = e - r * npad;
        float d = 0.f;
        if (c == 0 && r < nv) {
            const float diff = S.outb[r * S.op] - target[idx[r]];
            d = scale * (2.f * diff * invm);
            loss += diff * diff;
        }
        S.outb[r * S.op + c] = d;
    }
    __syncthreads();
}
// the same for one row of a critic with a TD loss kind and several target columns y_j, j in [c0, c1) (MAPPO.py:418-436: v_s repeated n
// times).  ValueClip is absent on purpose: torch.max(original.mean(), clipped.mean()) always steps like, and reports, the original
// loss (DESIGN.md "MAPPO / IPPO").  Adds sum_j l(y_j - v) to `loss`, returns d (that sum) / d v.
__device__ __forceinline__ float value_row(const LearnArgs& la, float v, g_cf vt_row, int c0, int c1, float& loss) {
    float dv = 0.f;
    for (int j = c0; j < c1; ++j) {
        float l, g;
        td_loss_row(la, vt_row[j] - v, l, g);
        loss += l;
        dv -= g;
    }
    return dv;
}

// ---- advantage normalisation (PPO_with_tricks.py:314-315, PPO2.py:186-233, MAPPO.py:385-386, IPPO.py:270-271): adv[at(k)] = (raw[at(k)] -
// mean) / (std + 1e-8) over k < cnt with the unbiased std.  `s1` is the thread's partial sum of the raw values, accumulated by the
// caller in its own order (that order decides the mean's bits); `red` is block_sum's scratch.
template <class At>
__device__ __forceinline__ void normalize_adv(float s1, int cnt, g_cf raw, g_f adv, At at, lds_f red) {
    const float mean = block_sum(s1, red) / (float)cnt;
    float s2 = 0.f;
    for (int k = threadIdx.x; k < cnt; k += kWG) {
        const float d = raw[at(k)] - mean;
        s2 += d * d;
    }
    const float sd = sqrtf(block_sum(s2, red) / (float)(cnt - 1));
    for (int k = threadIdx.x; k < cnt; k += kWG) adv[at(k)] = (raw[at(k)] - mean) / (sd + 1e-8f);
}

}  // namespace frl
