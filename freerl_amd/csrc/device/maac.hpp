// MAAC's attention critic (MAAC_file/Attention.py:63-231, is_continue = False) on one 16-row chunk: forward and closed-form backward.
//
//     s_i = lrelu(encoder_fc_s o_i)                     Q = query(s_i)
//     e_j = lrelu(encoder_fc_sa_j [o_j | a_j])          for the others j != i, encoder_fc_sa_j from agent j's ONLINE critic
//     K_j = key(e_j)    V_j = lrelu(value(e_j))         attn_h = sum_j softmax_j(<Q_h, K_jh> / sqrt(d)) V_jh,  d = hidden / 4
//     all_q = fc2(lrelu(fc1([s_i | fc_out(attn)])))     one value per action of agent i
//
// The others are STREAMED through the chunk, as device/mappo_att.hpp streams them: one [o_j | a_j] segment (xin), one e_j (h1) and one
// [K_j | Vpre_j] (kv) are alive at a time whatever n_agents is; what stays per row is the 4 (n - 1) raw scores and, per head, the online
// softmax's running max m, sum l and weighted V.  The backward streams them a second time with p = exp(s - m) / l:
//     d V_jh = p d attn_h (through the LeakyReLU slope)     d s = p (<d attn_h, V_jh> - D_h) / sqrt(d),  D_h = <d attn_h, attn_h>
//     d K_jh = d s Q_h      d Q_h += d s K_jh
// written in place over [K_j | Vpre_j]: the stacked layer's dW is ONE linear_bwd_dw.  Nothing flows into e_j's encoder (it is another
// agent's layer, and agent i's optimiser does not hold it).
// Where the data lives: every matrix product is net.hpp's MFMA linear_fwd / linear_bwd_* on LDS rows (the 16 rows are the M tile); a
// (row, head) pair belongs to 16 lanes of one wave, two of the head's d <= 32 columns each (lanes past d / 2 add zeros), and its dot
// products are a fixed four-step butterfly over those lanes: the same bits on every run.
// The attention block is EngineDesc::maac_att (query, [key | value], fc_out); critic i's own layers are net 2i+1 (MaacLayer).
#pragma once
#include "update_common.hpp"

namespace frl {

struct MaacLds {
    lds_f xcat, kv, dx; int cp;                  // [rc][2 hidden + 4]: [s_i | fc_out(attn)], [K_j | Vpre_j] then their deltas, d xcat
    lds_f Q, attn, dattn, dQ, ds;                // [rc][hidden + 4]
    lds_f sc; int sp;                            // [rc][4 (n_agents - 1)] raw scaled scores, other jj's four heads at [4 jj, 4 jj + 4)
    lds_f ml;                                    // [rc][8] m then l per head
    lds_f Dh;                                    // [rc][4]
    int hd;                                      // columns of a head
    float scale;                                 // 1 / sqrt(hd)
};

// must mirror frl_desc.h: maac_row_extra()
__device__ __forceinline__ MaacLds carve_maac(const Lds& S, int n_agents) {
    MaacLds A;
    const int rc = S.rc, H = S.hp - 4;
    A.cp = 2 * H + 4;
    A.sp = kMaacHeads * (n_agents - 1);
    A.hd = H / kMaacHeads;
    A.scale = 1.f / sqrtf((float)A.hd);
    lds_f p = S.red + 8;
    A.xcat = p; p += rc * A.cp;
    A.kv = p; p += rc * A.cp;
    A.dx = p; p += rc * A.cp;
    A.Q = p; p += rc * S.hp;
    A.attn = p; p += rc * S.hp;
    A.dattn = p; p += rc * S.hp;
    A.dQ = p; p += rc * S.hp;
    A.ds = p; p += rc * S.hp;
    A.sc = p; p += rc * A.sp;
    A.ml = p; p += rc * 8;
    A.Dh = p;
    return A;
}

// The chunk's rows: rows idx[0 .. nv) of a ring, or (idx null) the nv consecutive rows at src.  Either way a row starts
// [obs_0 .. obs_{n-1} | act_0 .. act_{n-1}] at the record's column offsets (a ring row goes on; next = 1 reads its next_obs blocks instead).
// ab: the others' actions come from the chunk's abuf (fresh draws, one-hot) instead of the rows' own action blocks
struct MaacRows { g_cf src; g_ci idx; int stride, nv, next; lds_cf ab; };
__device__ __forceinline__ size_t maac_row(const MaacRows& R, int r) { return (size_t)(R.idx ? R.idx[r] : r) * R.stride; }

// xin <- [o_j | a_j] of the chunk's rows (A = 0: the observation alone); zeros in invalid rows and up to kpad
__device__ __forceinline__ void maac_load_seg(const RecordDesc& Rd, const Lds& S, const MaacRows& R, int j, bool with_action, int kpad) {
    const int O = Rd.obs_dim[j], A = with_action ? Rd.act_dim[j] : 0;
    const int ocol = R.next ? Rd.nobs_off[j] : Rd.obs_off[j], acol = Rd.act_off[j], cj = Rd.act_off[j] - Rd.act_off[0];
    for (int e = threadIdx.x; e < S.rc * kpad; e += kWG) {
        const int r = e / kpad, c = e - r * kpad;
        float v = 0.f;
        if (r < R.nv) {
            if (c < O) v = R.src[maac_row(R, r) + ocol + c];
            else if (c < O + A) v = R.ab ? R.ab[r * S.ap + cj + c - O] : R.src[maac_row(R, r) + acol + c - O];
        }
        S.xin[r * S.xp + c] = v;
    }
}

// f(row, head, li, on): the (row, head) pairs of a chunk, 16 lanes each; lane li owns columns hd * head + 2 li, + 1 while 2 li < hd (on).
// Every lane of every wave makes the same number of trips, so the butterflies below run with all lanes active
template <class F>
__device__ __forceinline__ void maac_pairs(int rc, int hd, F f) {
    const int li = threadIdx.x & 15;
    for (int pr = threadIdx.x >> 4; pr < rc * kMaacHeads; pr += kWG / 16) f(pr >> 2, pr & 3, li, 2 * li < hd);
}
__device__ __forceinline__ float maac_sum16(float v) {
    v += lane_xor(v, 1); v += lane_xor(v, 2); v += lane_xor(v, 4); v += lane_xor(v, 8);
    return v;
}
__device__ __forceinline__ float maac_leaky(float x) { return x > 0.f ? x : kLeakySlope * x; }
__device__ __forceinline__ float maac_slope(float x) { return x > 0.f ? 1.f : kLeakySlope; }
// a lane's two columns of a dot product, in ONE written-out rounding order: <d attn, V_j> and D_h = <d attn, attn> must agree to the bit
// when attn IS V_j (one other agent), so that d s — and with it the key's and the query's gradient — is exactly zero there
__device__ __forceinline__ float maac_dot2(float a0, float b0, float a1, float b1) { return __fmaf_rn(a0, b0, __fmul_rn(a1, b1)); }

// one streamed other (the jj-th) of the forward: its scores, and the online softmax's m, l and weighted V per head
__device__ __forceinline__ void maac_attend(const Lds& S, const MaacLds& A, int jj) {
    const int H = S.hp - 4;
    maac_pairs(S.rc, A.hd, [&](int r, int h, int li, bool on) {
        const int c = on ? A.hd * h + 2 * li : 0;
        lds_cf q = A.Q + r * S.hp + c;
        lds_cf kv = A.kv + r * A.cp + c;
        const float s = maac_sum16(on ? maac_dot2(q[0], kv[0], q[1], kv[1]) : 0.f) * A.scale;
        lds_f ml = A.ml + r * 8;
        lds_f at = A.attn + r * S.hp + c;
        const float m0 = jj ? ml[h] : s, l0 = jj ? ml[4 + h] : 0.f;
        const float m1 = fmaxf(m0, s), al = expf(m0 - m1), pw = expf(s - m1);
        if (on) {
            const float a0 = jj ? at[0] : 0.f, a1 = jj ? at[1] : 0.f;
            at[0] = __fmaf_rn(pw, maac_leaky(kv[H]), __fmul_rn(a0, al));
            at[1] = __fmaf_rn(pw, maac_leaky(kv[H + 1]), __fmul_rn(a1, al));
        }
        if (li == 0) { A.sc[r * A.sp + 4 * jj + h] = s; ml[h] = m1; ml[4 + h] = l0 * al + pw; }
    });
}

// ... and of the backward: [K_j | Vpre_j] -> [d K_j | d Vpre_j] in place, d Q accumulated
__device__ __forceinline__ void maac_attend_bwd(const Lds& S, const MaacLds& A, int jj) {
    const int H = S.hp - 4;
    maac_pairs(S.rc, A.hd, [&](int r, int h, int li, bool on) {
        const int c = on ? A.hd * h + 2 * li : 0;
        lds_f kv = A.kv + r * A.cp + c;
        lds_cf q = A.Q + r * S.hp + c;
        lds_cf da = A.dattn + r * S.hp + c;
        lds_f dq = A.dQ + r * S.hp + c;
        const float p = expf(A.sc[r * A.sp + 4 * jj + h] - A.ml[r * 8 + h]) / A.ml[r * 8 + 4 + h];
        const float vp0 = kv[H], vp1 = kv[H + 1];
        const float t = maac_sum16(on ? maac_dot2(da[0], maac_leaky(vp0), da[1], maac_leaky(vp1)) : 0.f);
        const float ds = p * (t - A.Dh[r * 4 + h]) * A.scale;
        if (on) {
            dq[0] += ds * kv[0];
            dq[1] += ds * kv[1];
            kv[0] = ds * q[0];
            kv[1] = ds * q[1];
            kv[H] = p * da[0] * maac_slope(vp0);
            kv[H + 1] = p * da[1] * maac_slope(vp1);
        }
    });
}

// Critic i of one learner: its own layers (net 2i+1) from thC, the attention block from thA, the others' encoder_fc_sa from the
// learner's ONLINE parameters th_online (also under a target critic: Attention.py reads agents[j].critic)
struct MaacCritic { const NetDesc& NC; const NetDesc& NA; g_cf thC, thA, th_online; int i; };

// all_q of the chunk's rows into outb (A_i columns).  Leaves for the backward: s_i and fc_out's output in xcat, Q, the normalised attn,
// the scores with m and l, fc1's activation in h2.  Ends with a barrier.
__device__ __noinline__ void maac_fwd(const EngineDesc& D, const MaacCritic& C, const Lds& S, const MaacLds& A, const MaacRows& R) {
    const int n = D.n_agents, H = S.hp - 4, rc = S.rc, i = C.i;
    maac_load_seg(D.rec, S, R, i, false, C.NC.L[MAAC_ENC_S].k_pad);
    FRL_PHASE(S);
    linear_fwd<true>(C.NC.L[MAAC_ENC_S], C.thC, S.xin, S.xp, A.xcat, A.cp, ACT_LEAKY_RELU, rc);
    FRL_PHASE(S);
    linear_fwd(C.NA.L[MAAC_Q], C.thA, A.xcat, A.cp, A.Q, S.hp, ACT_NONE, rc);
    for (int j = 0, jj = 0; j < n; ++j) {
        if (j == i) continue;
        const LayerDesc& E = D.net[2 * j + 1].L[MAAC_ENC_SA];
        maac_load_seg(D.rec, S, R, j, true, E.k_pad);
        FRL_PHASE(S);
        linear_fwd<true>(E, C.th_online + D.net_off[2 * j + 1], S.xin, S.xp, S.h1, S.hp, ACT_LEAKY_RELU, rc);
        FRL_PHASE(S);
        linear_fwd(C.NA.L[MAAC_KV], C.thA, S.h1, S.hp, A.kv, A.cp, ACT_NONE, rc);
        FRL_PHASE(S);
        maac_attend(S, A, jj++);
        FRL_PHASE(S);
    }
    maac_pairs(rc, A.hd, [&](int r, int h, int li, bool on) {
        if (!on) return;
        lds_f at = A.attn + r * S.hp + A.hd * h + 2 * li;
        const float l = A.ml[r * 8 + 4 + h];
        at[0] /= l;
        at[1] /= l;
    });
    FRL_PHASE(S);
    linear_fwd(C.NA.L[MAAC_O], C.thA, A.attn, S.hp, A.xcat + H, A.cp, ACT_NONE, rc);
    FRL_PHASE(S);
    linear_fwd<true>(C.NC.L[MAAC_FC1], C.thC, A.xcat, A.cp, S.h2, S.hp, ACT_LEAKY_RELU, rc);
    FRL_PHASE(S);
    linear_fwd(C.NC.L[MAAC_FC2], C.thC, S.h2, S.hp, S.outb, S.op, ACT_NONE, rc);
    FRL_PHASE(S);
}

// Backward of the same: d loss / d all_q in outb (zero in its pad columns and in invalid rows); the gradients of the own net's
// encoder_fc_s, fc1, fc2 to G and of the attention block to GA (gs: GS_STORE for a workgroup's first chunk, GS_ADD after it — the
// [key | value] layer is added to once per other agent, so a chunk never streams: RowUnit::walk(rows, true)).  The query's and the
// key's bias slots receive column sums no optimiser reads (maac_trained_at skips them).  Ends with a barrier.
__device__ __noinline__ void maac_bwd(const EngineDesc& D, const MaacCritic& C, g_f G, g_f GA, const Lds& S, const MaacLds& A, const MaacRows& R,
                                         int gs) {
    const int n = D.n_agents, H = S.hp - 4, rc = S.rc, ht = H / 16, i = C.i;
    linear_bwd_dw(C.NC.L[MAAC_FC2], G, S.outb, S.op, S.h2, S.hp, rc, gs);
    FRL_PHASE(S);
    linear_bwd_dx<true>(C.NC.L[MAAC_FC2], C.thC, S.outb, S.op, S.h2, S.hp, ACT_LEAKY_RELU, rc, 0, ht);
    FRL_PHASE(S);
    linear_bwd_dw(C.NC.L[MAAC_FC1], G, S.h2, S.hp, A.xcat, A.cp, rc, gs);
    linear_bwd_dx(C.NC.L[MAAC_FC1], C.thC, S.h2, S.hp, A.dx, A.cp, ACT_NONE, rc, 0, 2 * ht);      // [d s_i | d other]
    FRL_PHASE(S);
    linear_bwd_dw(C.NA.L[MAAC_O], GA, A.dx + H, A.cp, A.attn, S.hp, rc, gs);
    linear_bwd_dx(C.NA.L[MAAC_O], C.thA, A.dx + H, A.cp, A.dattn, S.hp, ACT_NONE, rc, 0, ht);
    FRL_PHASE(S);
    maac_pairs(rc, A.hd, [&](int r, int h, int li, bool on) {
        const int c = on ? A.hd * h + 2 * li : 0;
        lds_cf da = A.dattn + r * S.hp + c;
        lds_cf at = A.attn + r * S.hp + c;
        const float d = maac_sum16(on ? maac_dot2(da[0], at[0], da[1], at[1]) : 0.f);
        if (li == 0) A.Dh[r * 4 + h] = d;
        if (on) {
            A.dQ[r * S.hp + c] = 0.f;
            A.dQ[r * S.hp + c + 1] = 0.f;
        }
    });
    for (int j = 0, jj = 0; j < n; ++j) {
        if (j == i) continue;
        const LayerDesc& E = D.net[2 * j + 1].L[MAAC_ENC_SA];
        maac_load_seg(D.rec, S, R, j, true, E.k_pad);
        FRL_PHASE(S);
        linear_fwd<true>(E, C.th_online + D.net_off[2 * j + 1], S.xin, S.xp, S.h1, S.hp, ACT_LEAKY_RELU, rc);
        FRL_PHASE(S);
        linear_fwd(C.NA.L[MAAC_KV], C.thA, S.h1, S.hp, A.kv, A.cp, ACT_NONE, rc);
        FRL_PHASE(S);
        maac_attend_bwd(S, A, jj);
        FRL_PHASE(S);
        linear_bwd_dw(C.NA.L[MAAC_KV], GA, A.kv, A.cp, S.h1, S.hp, rc, jj == 0 ? gs : GS_ADD);
        FRL_PHASE(S);
        ++jj;
    }
    maac_load_seg(D.rec, S, R, i, false, C.NC.L[MAAC_ENC_S].k_pad);
    linear_bwd_dw(C.NA.L[MAAC_Q], GA, A.dQ, S.hp, A.xcat, A.cp, rc, gs, false);
    linear_bwd_dx(C.NA.L[MAAC_Q], C.thA, A.dQ, S.hp, A.ds, S.hp, ACT_NONE, rc, 0, ht);
    FRL_PHASE(S);
    for (int e = threadIdx.x; e < rc * H; e += kWG) {                                      // d s_i = (fc1's part + Wq^T d Q) through the LeakyReLU
        const int r = e / H, c = e - r * H;
        A.ds[r * S.hp + c] = (A.ds[r * S.hp + c] + A.dx[r * A.cp + c]) * maac_slope(A.xcat[r * A.cp + c]);
    }
    FRL_PHASE(S);
    linear_bwd_dw(C.NC.L[MAAC_ENC_S], G, A.ds, S.hp, S.xin, S.xp, rc, gs);
    FRL_PHASE(S);
}

// ---- Actor_discrete's head (MAAC_discrete.py:51-75) on a row of logits: softmax, Categorical's renormalisation and torch.multinomial's
// single-sample rule argmax_k probs[k] / q[k], q ~ Exp(1) (the first of equal ratios, as argmax)
struct MaacSoftmax { float zmax, ssum, psum; };
__device__ __forceinline__ MaacSoftmax maac_softmax(lds_cf z, int A) {
    MaacSoftmax m{z[0], 0.f, 0.f};
    for (int c = 1; c < A; ++c) m.zmax = fmaxf(m.zmax, z[c]);
    for (int c = 0; c < A; ++c) m.ssum += expf(z[c] - m.zmax);
    for (int c = 0; c < A; ++c) m.psum += expf(z[c] - m.zmax) / m.ssum;
    return m;
}
__device__ __forceinline__ float maac_prob(const MaacSoftmax& m, float z) { return expf(z - m.zmax) / m.ssum; }
__device__ __forceinline__ float maac_logp(const MaacSoftmax& m, float z) { return (z - m.zmax) - logf(m.ssum); }
__device__ __forceinline__ int maac_draw(const MaacSoftmax& m, lds_cf z, int A, g_cf q) {
    int k = 0;
    float best = 0.f;
    for (int c = 0; c < A; ++c) {
        const float ratio = (maac_prob(m, z[c]) / m.psum) / q[c];
        if (c == 0 || ratio > best) { best = ratio; k = c; }
    }
    return k;
}

// The 12 tensors agent i's optimiser steps, as ONE index space of float4: element v of it lies off4 float4 into critic i's own net
// (att = false: encoder_fc_s, fc1, fc2, weight and bias each) or into an attention slot (att = true: the query's weight, the [key | value]
// weight, the value's bias, fc_out's weight and bias).  The frozen eight (encoder_fc_sa, encoder_fc_a, bias_fc1, bias_fc2) and the bias
// slots the query and the key do not have are in no range: nothing reads or writes them.
__device__ __forceinline__ int maac_layer_span(const LayerDesc& L) { return L.b_off + L.n_pad - L.w_off; }
__device__ __forceinline__ int maac_trained4(const NetDesc& NC, const NetDesc& NA) {
    const int H = NA.L[MAAC_Q].n_pad;
    return (maac_layer_span(NC.L[MAAC_ENC_S]) + maac_layer_span(NC.L[MAAC_FC1]) + maac_layer_span(NC.L[MAAC_FC2]) + H * H + 2 * H * H + H +
            maac_layer_span(NA.L[MAAC_O])) / 4;
}
__device__ __forceinline__ void maac_trained_at(const NetDesc& NC, const NetDesc& NA, int v, int& off4, bool& att) {
    const int H = NA.L[MAAC_Q].n_pad;
    const int off[7] = {NC.L[MAAC_ENC_S].w_off, NC.L[MAAC_FC1].w_off, NC.L[MAAC_FC2].w_off, NA.L[MAAC_Q].w_off, NA.L[MAAC_KV].w_off, NA.L[MAAC_KV].b_off + H,
                        NA.L[MAAC_O].w_off};
    const int len[7] = {maac_layer_span(NC.L[MAAC_ENC_S]), maac_layer_span(NC.L[MAAC_FC1]), maac_layer_span(NC.L[MAAC_FC2]), H * H, 2 * H * H, H,
                        maac_layer_span(NA.L[MAAC_O])};
    off4 = 0;
    att = false;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int l4 = len[k] / 4;
        if (v >= 0 && v < l4) { off4 = off[k] / 4 + v; att = k >= 3; }
        v -= l4;
    }
}

}  // namespace frl
