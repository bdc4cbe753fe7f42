// The attention critic of ATT-MADDPG (MADDPG_file/ATT.py:81-103,181-229) on the row-chunk primitives of net.hpp: its LDS carve, the
// forward and the backward of one row chunk.  Per row, for agent i's critic (H = hidden, K = kAttHeads):
//     x_e = [o_0 | .. | o_{n-1} | a_i]      x_d = [a_j, j != i]
//     e = W_E x_e + b_E      d = W_D x_d + b_D                       (no activation)
//     g = relu(W_ei e + b_ei)     h_k = relu(W_k g + b_k)     u = relu(W_di d + b_di)
//     s_k = <h_k, u>    p = softmax_k(s)    c = sum_k p_k h_k
//     y = relu(W_1 c + b_1)    Q = W_2 y + b_2
// The ten nn.Linear are seven layers (frl_desc.h: AttLayer, the heads stacked into one 4 H-wide layer) and go through linear_fwd /
// linear_bwd_dw / linear_bwd_dx; the scores, the softmax and the weighted sum are VALU work, one wave per row with a wave reduction
// over H.  Every tensor of the chunk stays in LDS and is overwritten by its delta on the way back, as in mlp_bwd:
//     xin = x_e   h1 = e   h2 = g   outb = Q / its delta          (the common carve: the actors' mlp_fwd / mlp_bwd use the same buffers)
//     xd, d, u, c, yh, hk                                          (carve_att, behind it: EngineDesc::lds_row_extra floats per row)
// and the softmax weights p[rc][K] sit in S.y behind the chunk's TD targets.
#pragma once
#include "net.hpp"

namespace frl {

struct AttLds {
    lds_f xd; int dp;      // [rc][dp] x_d, zero padded to the decoder layer's k_pad
    lds_f d, u, c, yh;     // [rc][hp] each
    lds_f hk; int kp;      // [rc][kp] the K heads of a row side by side: h_k at columns [k H, (k + 1) H)
    lds_f p;               // [rc][K] softmax weights
};
constexpr int kAttPOff = 32;      // floats into S.y where p starts: S.y[0 .. rc) are the TD targets, rc = kAttRc = 16, lds_batch_pad = 128

// must mirror engine_plan.hpp: lds_bytes_for() with lds_row_extra = att_row_extra(hidden, xd_pad)
__device__ __forceinline__ AttLds carve_att(const EngineDesc& D, const Lds& S, float* smem) {
    AttLds A;
    const int rc = D.rc, H = D.hidden;
    A.dp = D.lds_row_extra - 4 * (H + 4) - (kAttHeads * H + 4);
    A.kp = kAttHeads * H + 4;
    lds_f p = (lds_f)smem + rc * (S.xp + D.lds_hbufs * S.hp + S.op + 2 * S.ap) + D.lds_batch_pad + 8;
    A.xd = p; p += rc * A.dp;
    A.d = p; p += rc * S.hp;
    A.u = p; p += rc * S.hp;
    A.c = p; p += rc * S.hp;
    A.yh = p; p += rc * S.hp;
    A.hk = p;
    A.p = S.y + kAttPOff;
    return A;
}

// scores, softmax over the K heads (max-subtracted, as torch's), weighted sum: one wave per row
__device__ __forceinline__ void att_attend(const Lds& S, const AttLds& A, int H) {
    const int w = wave_id(), l = lane_id();
    for (int r = w; r < S.rc; r += kWaves) {
        lds_cf hk = A.hk + r * A.kp;
        lds_cf u = A.u + r * S.hp;
        float s[kAttHeads];
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) s[k] = 0.f;
        for (int c = l; c < H; c += 64) {
            const float uc = u[c];
#pragma unroll
            for (int k = 0; k < kAttHeads; ++k) s[k] += hk[k * H + c] * uc;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) { s[k] = wave_sum(s[k]); mx = fmaxf(mx, s[k]); }
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) { s[k] = expf(s[k] - mx); sum += s[k]; }
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) s[k] = s[k] / sum;
        for (int c = l; c < H; c += 64) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < kAttHeads; ++k) acc += s[k] * hk[k * H + c];
            A.c[r * S.hp + c] = acc;
        }
        if (l == 0) st4(A.p + r * kAttHeads, f32x4{s[0], s[1], s[2], s[3]});
    }
}

// dc in A.c, p in A.p, h_k and u as the forward left them -> dh_k (ReLU mask applied) over h_k, du (masked) over u:
//     dp_k = <dc, h_k>    ds_k = p_k (dp_k - sum_j p_j dp_j)    dh_k = p_k dc + ds_k u    du = sum_k ds_k h_k
__device__ __forceinline__ void att_attend_bwd(const Lds& S, const AttLds& A, int H) {
    const int w = wave_id(), l = lane_id();
    for (int r = w; r < S.rc; r += kWaves) {
        lds_f hk = A.hk + r * A.kp;
        lds_f u = A.u + r * S.hp;
        lds_cf dc = A.c + r * S.hp;
        const f32x4 p = ld4((lds_cf)(A.p + r * kAttHeads));
        float dp[kAttHeads];
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) dp[k] = 0.f;
        for (int c = l; c < H; c += 64) {
            const float dcc = dc[c];
#pragma unroll
            for (int k = 0; k < kAttHeads; ++k) dp[k] += hk[k * H + c] * dcc;
        }
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) { dp[k] = wave_sum(dp[k]); dot += p[k] * dp[k]; }
        float ds[kAttHeads];
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) ds[k] = p[k] * (dp[k] - dot);
        for (int c = l; c < H; c += 64) {
            const float dcc = dc[c], uc = u[c];
            float du = 0.f;
#pragma unroll
            for (int k = 0; k < kAttHeads; ++k) {
                const float h = hk[k * H + c];
                du += ds[k] * h;
                hk[k * H + c] = h > 0.f ? p[k] * dcc + ds[k] * uc : 0.f;
            }
            u[c] = uc > 0.f ? du : 0.f;
        }
    }
}

// Forward of net N (an attention critic) with parameters theta on x_e in S.xin and x_d in A.xd, both zero padded to their layers' k_pad:
// Q of row r in S.outb[r * S.op].  Six barrier phases; ends with a barrier.
__device__ __attribute__((noinline)) void att_fwd(const NetDesc& N, g_cf theta, const Lds& S, const AttLds& A) {
    const int rc = S.rc, H = N.L[ATT_EI].n;
    linear_fwd(N.L[ATT_E], theta, S.xin, S.xp, S.h1, S.hp, ACT_NONE, rc);
    linear_fwd(N.L[ATT_D], theta, A.xd, A.dp, A.d, S.hp, ACT_NONE, rc);
    FRL_PHASE(S);
    linear_fwd(N.L[ATT_EI], theta, S.h1, S.hp, S.h2, S.hp, ACT_RELU, rc);
    linear_fwd(N.L[ATT_DI], theta, A.d, S.hp, A.u, S.hp, ACT_RELU, rc);
    FRL_PHASE(S);
    linear_fwd(N.L[ATT_HEADS], theta, S.h2, S.hp, A.hk, A.kp, ACT_RELU, rc);
    FRL_PHASE(S);
    att_attend(S, A, H);
    FRL_PHASE(S);
    linear_fwd(N.L[ATT_FC1], theta, A.c, S.hp, A.yh, S.hp, ACT_RELU, rc);
    FRL_PHASE(S);
    linear_fwd(N.L[ATT_FC2], theta, A.yh, S.hp, S.outb, S.op, ACT_NONE, rc);
    FRL_PHASE(S);
}

// Backward of att_fwd: head delta in S.outb (zero in the padded columns and the invalid rows).  G != nullptr: every layer's weight /
// bias gradient goes to G the way `gs` says (net.hpp: GradStore), both branches.  G == nullptr: the input gradient only, down the
// encoder branch (the decoder branch has no backward then), and want_dx0 leaves d loss / d x_e in S.xin for column tiles [ct0, ct1).
// Ends with a barrier.
__device__ __attribute__((noinline)) void att_bwd(const NetDesc& N, g_cf theta, g_f G, const Lds& S, const AttLds& A, int gs, bool want_dx0, int ct0, int ct1) {
    const int rc = S.rc, H = N.L[ATT_EI].n, ht = H / 16;
    if (G) { linear_bwd_dw(N.L[ATT_FC2], G, S.outb, S.op, A.yh, S.hp, rc, gs); FRL_PHASE(S); }
    linear_bwd_dx(N.L[ATT_FC2], theta, S.outb, S.op, A.yh, S.hp, ACT_RELU, rc, 0, ht);
    FRL_PHASE(S);
    if (G) { linear_bwd_dw(N.L[ATT_FC1], G, A.yh, S.hp, A.c, S.hp, rc, gs); FRL_PHASE(S); }
    linear_bwd_dx(N.L[ATT_FC1], theta, A.yh, S.hp, A.c, S.hp, ACT_NONE, rc, 0, ht);
    FRL_PHASE(S);
    att_attend_bwd(S, A, H);
    FRL_PHASE(S);
    if (G) {
        linear_bwd_dw(N.L[ATT_HEADS], G, A.hk, A.kp, S.h2, S.hp, rc, gs);
        linear_bwd_dw(N.L[ATT_DI], G, A.u, S.hp, A.d, S.hp, rc, gs);
        FRL_PHASE(S);
    }
    linear_bwd_dx(N.L[ATT_HEADS], theta, A.hk, A.kp, S.h2, S.hp, ACT_RELU, rc, 0, ht);
    if (G) linear_bwd_dx(N.L[ATT_DI], theta, A.u, S.hp, A.d, S.hp, ACT_NONE, rc, 0, ht);
    FRL_PHASE(S);
    if (G) {
        linear_bwd_dw(N.L[ATT_EI], G, S.h2, S.hp, S.h1, S.hp, rc, gs);
        linear_bwd_dw(N.L[ATT_D], G, A.d, S.hp, A.xd, A.dp, rc, gs);
        FRL_PHASE(S);
    }
    linear_bwd_dx(N.L[ATT_EI], theta, S.h2, S.hp, S.h1, S.hp, ACT_NONE, rc, 0, ht);
    FRL_PHASE(S);
    if (G) { linear_bwd_dw(N.L[ATT_E], G, S.h1, S.hp, S.xin, S.xp, rc, gs); FRL_PHASE(S); }
    if (want_dx0) {
        linear_bwd_dx(N.L[ATT_E], theta, S.h1, S.hp, S.xin, S.xp, ACT_NONE, rc, ct0, ct1);
        FRL_PHASE(S);
    }
}

// x_d of agent `ag` from a row's actions of ALL agents at src[r * lds + .] (act_total columns, agent order): the columns in front of
// the agent's own block, then the ones behind it; zero up to the decoder layer's k_pad
__device__ __forceinline__ void att_fill_xd(const AttLds& A, int rc, lds_cf src, int lds, int a0, int Aa, int AT, int kd) {
    for (int e = threadIdx.x; e < rc * kd; e += kWG) {
        const int r = e / kd, c = e - r * kd;
        A.xd[r * A.dp + c] = c < AT - Aa ? src[r * lds + (c < a0 ? c : c + Aa)] : 0.f;
    }
}

}  // namespace frl
