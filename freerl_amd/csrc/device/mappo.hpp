// MAPPO / IPPO device code (MAPPO_file/MAPPO.py, IPPO.py): the normalised forward and backward of one row chunk, and the per-row
// head arithmetic of the clipped surrogate and of the critic's regression over one or n_agents advantage / target columns.
//
// Forward: [feature_norm] -> l1 -> ReLU -> [LN] -> l2 -> ReLU -> [LN] -> head, both norms F.layer_norm without affine part, biased
// variance, eps 1e-5.  Without LayerNorm this is device/net.hpp's mlp_fwd / mlp_bwd as they are (feature_norm rewrites xin only and
// needs no backward: it is the input).  With it a hidden layer keeps its NORMALISED row in h1 / h2 (the next layer's input and the
// xhat of the LayerNorm backward), one rstd per row, and its ReLU mask as one bit per unit; the backward of a layer is
//     dn = dY W  (plain)  ->  da = rstd (dn - mean(dn) - xhat mean(dn xhat))  ->  dz = da where the unit was positive
// with dn written to a third hidden buffer (dbuf) so that xhat survives until the row's two means are taken.  One wave walks a row and
// both means are a fixed butterfly over its 64 lanes: the same bits on every run.
#pragma once
#include "net.hpp"

namespace frl {

constexpr float kLnEps = 1e-5f;          // F.layer_norm's default

struct MappoLds {
    lds_f dbuf;                  // [rc][hp] d loss / d (normalised row), then the layer's delta
    lds_f rstd;                  // [2][rc]
    FRL_LDS unsigned* mask;      // [2][rc][kMappoMaskWords]
};

__device__ __forceinline__ MappoLds carve_mappo(const Lds& S) {
    MappoLds X;
    lds_f p = S.red + 8;
    X.dbuf = p; p += S.rc * S.hp;
    X.rstd = p; p += 2 * S.rc;
    X.mask = (FRL_LDS unsigned*)p;
    return X;
}

// x <- (x - mean) / sqrt(var + eps) over the first n columns of every row; one wave per row.  bits != nullptr: bit c of the row's mask
// = (x[c] > 0) BEFORE the normalisation (the ReLU that produced x passes gradient there); rs != nullptr: the row's rstd.
__device__ __forceinline__ void ln_rows(lds_f X, int ldx, int n, int rc, lds_f rs, FRL_LDS unsigned* bits) {
    const int l = lane_id(), w = wave_id();
    const float inv = 1.f / (float)n;
    for (int r = w; r < rc; r += kWaves) {
        lds_f x = X + r * ldx;
        float s = 0.f;
        for (int c = l; c < n; c += 64) s += x[c];
        const float mean = wave_sum(s) * inv;
        float q = 0.f;
        for (int c = l; c < n; c += 64) { const float d = x[c] - mean; q += d * d; }
        const float rstd = 1.f / sqrtf(wave_sum(q) * inv + kLnEps);
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int c = c0 + l;
            const float v = c < n ? x[c] : 0.f;
            if (bits) {
                const unsigned long long b = __ballot(v > 0.f);
                if (l == 0) { bits[r * kMappoMaskWords + (c0 >> 5)] = (unsigned)b; bits[r * kMappoMaskWords + (c0 >> 5) + 1] = (unsigned)(b >> 32); }
            }
            if (c < n) x[c] = (v - mean) * rstd;
        }
        if (rs && l == 0) rs[r] = rstd;
    }
}

// dY (the gradient at the normalised row) -> the layer's delta, in place: through F.layer_norm, then the ReLU mask
__device__ __forceinline__ void ln_bwd_rows(lds_f dY, lds_cf Xhat, int ld, int n, int rc, lds_cf rs, const FRL_LDS unsigned* bits) {
    const int l = lane_id(), w = wave_id();
    const float inv = 1.f / (float)n;
    for (int r = w; r < rc; r += kWaves) {
        lds_f dy = dY + r * ld;
        lds_cf xh = Xhat + r * ld;
        float s1 = 0.f, s2 = 0.f;
        for (int c = l; c < n; c += 64) { const float g = dy[c]; s1 += g; s2 += g * xh[c]; }
        const float m1 = wave_sum(s1) * inv, m2 = wave_sum(s2) * inv, rstd = rs[r];
        for (int c = l; c < n; c += 64) {
            const bool open = (bits[r * kMappoMaskWords + (c >> 5)] >> (c & 31)) & 1u;
            dy[c] = open ? rstd * ((dy[c] - m1) - xh[c] * m2) : 0.f;
        }
    }
}

// Forward of a three-layer net on the chunk in xin (kin real input columns).  Ends with a barrier; the head's rows are in outb.
__device__ __forceinline__ void mappo_fwd(const EngineDesc& D, const NetDesc& N, g_cf theta, const Lds& S, const MappoLds& X, int kin,
                                          int out_act) {
    if (D.feature_norm) {
        ln_rows(S.xin, S.xp, kin, S.rc, nullptr, nullptr);
        FRL_PHASE(S);
    }
    if (!D.layer_norm) { mlp_fwd(N, 0, N.n_layers, theta, S, out_act); return; }
    const int H = N.L[0].n;
    linear_fwd(N.L[0], theta, S.xin, S.xp, S.h1, S.hp, ACT_RELU, S.rc);
    FRL_PHASE(S);
    ln_rows(S.h1, S.hp, H, S.rc, X.rstd, X.mask);
    FRL_PHASE(S);
    linear_fwd(N.L[1], theta, S.h1, S.hp, S.h2, S.hp, ACT_RELU, S.rc);
    FRL_PHASE(S);
    ln_rows(S.h2, S.hp, H, S.rc, X.rstd + S.rc, X.mask + S.rc * kMappoMaskWords);
    FRL_PHASE(S);
    linear_fwd(N.L[2], theta, S.h2, S.hp, S.outb, S.op, out_act, S.rc);
    FRL_PHASE(S);
}

// Backward of the same: head delta in outb (zero in padded columns and invalid rows), gradients to G as `gs` says.  Ends with a barrier.
__device__ __forceinline__ void mappo_bwd(const EngineDesc& D, const NetDesc& N, g_cf theta, g_f G, const Lds& S, const MappoLds& X, int gs) {
    if (!D.layer_norm) { mlp_bwd(N, 0, N.n_layers, theta, G, S, gs, false, 0, 0); return; }
    const int H = N.L[0].n;
    linear_bwd_dw(N.L[2], G, S.outb, S.op, S.h2, S.hp, S.rc, gs);
    linear_bwd_dx(N.L[2], theta, S.outb, S.op, X.dbuf, S.hp, ACT_NONE, S.rc, 0, N.L[2].k_pad / 16);
    FRL_PHASE(S);
    ln_bwd_rows(X.dbuf, S.h2, S.hp, H, S.rc, X.rstd + S.rc, X.mask + S.rc * kMappoMaskWords);
    FRL_PHASE(S);
    linear_bwd_dw(N.L[1], G, X.dbuf, S.hp, S.h1, S.hp, S.rc, gs);
    linear_bwd_dx(N.L[1], theta, X.dbuf, S.hp, S.h2, S.hp, ACT_NONE, S.rc, 0, N.L[1].k_pad / 16);      // (h2's xhat is spent)
    FRL_PHASE(S);
    ln_bwd_rows(S.h2, S.h1, S.hp, H, S.rc, X.rstd, X.mask);
    FRL_PHASE(S);
    linear_bwd_dw(N.L[0], G, S.h2, S.hp, S.xin, S.xp, S.rc, gs);
    FRL_PHASE(S);
}

// ---- per-row head arithmetic.  `adv` / `vt` point at the learner's [T][n_agents] matrices, row t's columns [c0, c1) take part:
// one column (the agent's own) on IPPO engines, all of them on MAPPO engines (MAPPO.py:410-412: ratios [m, 1] x adv[index] [m, n]).

// the clipped surrogate of one row: adds sum_j -min(ratio A_j, clamp(ratio) A_j) to `loss`, returns d (that sum) / d (sum of log-probs)
__device__ __forceinline__ float surrogate_row(float ratio, g_cf adv_row, int c0, int c1, float clip, float& loss) {
    float open = 0.f;
    for (int j = c0; j < c1; ++j) {
        const float A = adv_row[j];
        const float s1 = ratio * A, s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * A;
        loss += -fminf(s1, s2);
        open += s1 <= s2 ? A : 0.f;
    }
    return -open * ratio;
}

// the critic's regression of one row: v against the targets y_j (MAPPO.py:418-436: v_s repeated n times).  ValueClip is absent on
// purpose: torch.max(original.mean(), clipped.mean()) always steps like, and reports, the original loss (DESIGN.md "MAPPO / IPPO").
// Adds sum_j l(y_j - v) to `loss`, returns d (that sum) / d v.
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

}  // namespace frl
