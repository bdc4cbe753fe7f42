// MAPPO_attention's critic (MAPPO_file/attention.py:85-205) on one 16-row chunk: forward, closed-form backward and the 12-tensor Adam.
//
//     s   = [feature_norm over the whole joint observation]              s_j = agent j's slice of it
//     e_j = encoder_fc_s(s_j)   (agent i's own encoder for every j, no activation)
//     Q = query(e_i)    K_j = key(e_j)    V_j = LeakyReLU(value(e_j))    for the others j != i
//     attn_h = sum_j softmax_j(<Q_h, K_jh> / sqrt(32)) V_jh              per head h of 32 columns
//     V(s) = l3([LN] relu(l1([e_i | fc_out(attn)])))
//
// The others are STREAMED through the chunk: one observation segment, one e_j and one [K_j | Vpre_j] are alive at a time, whatever
// n_agents is; what stays per row is the 4 x (n - 1) raw scores and, per head, the online softmax's running max m, sum l and weighted V.
// The backward streams them a second time — e_j, K_j and Vpre_j are the weight gradients' operands anyway — with p = exp(s - m) / l:
//     d V_jh = p d attn_h (through the LeakyReLU slope)    d s = p (<d attn_h, V_jh> - D_h) / sqrt(32),  D_h = <d attn_h, attn_h>
//     d K_jh = d s Q_h     d Q_h += d s K_jh     d e_j = Wk^T d K_j + Wv^T d Vpre_j
// written IN PLACE over [K_j | Vpre_j], so that the stacked layer's dW and dX are one linear_bwd_dw / _dx each.
// Where the data lives: every matrix product is device/net.hpp's MFMA linear_fwd / linear_bwd_* on LDS rows (the 16 rows are the M
// tile); a (row, head) pair belongs to 16 lanes of one wave, two of the head's 32 columns each, and its dot products are a fixed
// four-step butterfly over those lanes: the same bits on every run.  The joint feature norm keeps a mean and an rstd per row and
// normalises a segment as it is loaded: the joint row itself (1440 columns at 8 x 180) is never resident.
// The attention block's parameters are net 1's (thA); gradients and Adam moments of all six layers are the critic's own net's.
#pragma once
#include "mappo.hpp"

namespace frl {

constexpr float kMattScale = 0.17677669529663687f;      // 1 / sqrt(32)

struct MattLds {
    lds_f xcat, kv, dx; int cp;                  // [rc][2 hidden + 4]: [e_i | fc_out(attn)], [K_j | Vpre_j] then their deltas, d xcat
    lds_f Q, attn, dattn, dQ, dej;               // [rc][hidden + 4]
    lds_f sc; int sp;                            // [rc][4 (n_agents - 1)] raw scaled scores, other jj's four heads at [4 jj, 4 jj + 4)
    lds_f ml;                                    // [rc][8] m then l per head
    lds_f Dh;                                    // [rc][4]
    lds_f fn;                                    // [rc][4] the joint feature norm's mean, rstd
};

// must mirror frl_desc.h: matt_row_extra()
__device__ __forceinline__ MattLds carve_matt(const Lds& S, int n_agents) {
    MattLds A;
    const int rc = S.rc, H = S.hp - 4;
    A.cp = 2 * H + 4;
    A.sp = kMattHeads * (n_agents - 1);
    lds_f p = S.red + 8 + rc * mappo_row_extra(H);
    A.xcat = p; p += rc * A.cp;
    A.kv = p; p += rc * A.cp;
    A.dx = p; p += rc * A.cp;
    A.Q = p; p += rc * S.hp;
    A.attn = p; p += rc * S.hp;
    A.dattn = p; p += rc * S.hp;
    A.dQ = p; p += rc * S.hp;
    A.dej = p; p += rc * S.hp;
    A.sc = p; p += rc * A.sp;
    A.ml = p; p += rc * 8;
    A.Dh = p; p += rc * 4;
    A.fn = p;
    return A;
}

// The chunk's rows: rows idx[0 .. nv) of src (a minibatch) or rows row0 .. row0 + nv - 1 (the value pass, frl_act)
struct MattRows { g_cf src; g_ci idx; int row0, stride, nv; };
__device__ __forceinline__ size_t matt_row(const MattRows& R, int r) { return (size_t)(R.idx ? R.idx[r] : R.row0 + r) * R.stride; }

// mean and rstd of F.layer_norm over columns [col0, col0 + width) of every valid row (ln_rows' arithmetic, read from global memory)
__device__ __forceinline__ void matt_row_stats(const MattLds& A, const MattRows& R, int col0, int width, int rc) {
    const int l = lane_id(), w = wave_id();
    const float inv = 1.f / (float)width;
    for (int r = w; r < rc; r += kWaves) {
        float mean = 0.f, rstd = 0.f;
        if (r < R.nv) {
            g_cf x = R.src + matt_row(R, r) + col0;
            float s = 0.f;
            for (int c = l; c < width; c += 64) s += x[c];
            mean = wave_sum(s) * inv;
            float q = 0.f;
            for (int c = l; c < width; c += 64) { const float d = x[c] - mean; q += d * d; }
            rstd = 1.f / sqrtf(wave_sum(q) * inv + kLnEps);
        }
        if (l == 0) { A.fn[4 * r] = mean; A.fn[4 * r + 1] = rstd; }
    }
}

// xin <- columns [col, col + O) of the chunk's rows, normalised with the row's joint statistics; zeros in invalid rows and pad columns
__device__ __forceinline__ void matt_load_seg(const Lds& S, const MattLds& A, const MattRows& R, int col, int O, int kpad, bool fnorm) {
    for (int e = threadIdx.x; e < S.rc * kpad; e += kWG) {
        const int r = e / kpad, c = e - r * kpad;
        float v = 0.f;
        if (r < R.nv && c < O) {
            v = R.src[matt_row(R, r) + col + c];
            if (fnorm) v = (v - A.fn[4 * r]) * A.fn[4 * r + 1];
        }
        S.xin[r * S.xp + c] = v;
    }
}

// f(row, head, li): the (row, head) pairs of a chunk, 16 lanes each (li = 0 .. 15 owns columns 32 head + 2 li, + 1); every lane of every
// wave makes the same number of trips, so the butterflies below run with all lanes active
template <class F>
__device__ __forceinline__ void matt_pairs(int rc, F f) {
    const int li = threadIdx.x & 15;
    for (int pr = threadIdx.x >> 4; pr < rc * kMattHeads; pr += kWG / 16) f(pr >> 2, pr & 3, li);
}
__device__ __forceinline__ float sum16(float v) {
    v += lane_xor<1>(v); v += lane_xor<2>(v); v += lane_xor<4>(v); v += lane_xor<8>(v);
    return v;
}
__device__ __forceinline__ float leaky(float x) { return x > 0.f ? x : kLeakySlope * x; }
// a lane's two columns of a dot product, in ONE written-out rounding order: <d attn, V_j> and D_h = <d attn, attn> must agree to the bit
// when attn IS V_j (one other agent), or d s = p (t - D_h) is rounding noise that Adam's division turns into a drift of query and key
__device__ __forceinline__ float dot2(float a0, float b0, float a1, float b1) { return __fmaf_rn(a0, b0, __fmul_rn(a1, b1)); }

// one streamed other (the jj-th) of the forward: its scores, and the online softmax's m, l and weighted V per head
__device__ __forceinline__ void matt_attend(const Lds& S, const MattLds& A, int jj) {
    const int H = S.hp - 4;
    matt_pairs(S.rc, [&](int r, int h, int li) {
        const int c = kMattHeadDim * h + 2 * li;
        lds_cf q = A.Q + r * S.hp + c;
        lds_cf kv = A.kv + r * A.cp + c;
        const float s = sum16(dot2(q[0], kv[0], q[1], kv[1])) * kMattScale;
        lds_f ml = A.ml + r * 8;
        lds_f at = A.attn + r * S.hp + c;
        const float m0 = jj ? ml[h] : s, l0 = jj ? ml[4 + h] : 0.f, a0 = jj ? at[0] : 0.f, a1 = jj ? at[1] : 0.f;
        const float m1 = fmaxf(m0, s), al = expf(m0 - m1), pw = expf(s - m1);
        at[0] = __fmaf_rn(pw, leaky(kv[H]), __fmul_rn(a0, al));
        at[1] = __fmaf_rn(pw, leaky(kv[H + 1]), __fmul_rn(a1, al));
        if (li == 0) { A.sc[r * A.sp + 4 * jj + h] = s; ml[h] = m1; ml[4 + h] = l0 * al + pw; }
    });
}

// ... and of the backward: [K_j | Vpre_j] -> [d K_j | d Vpre_j] in place, d Q accumulated
__device__ __forceinline__ void matt_attend_bwd(const Lds& S, const MattLds& A, int jj) {
    const int H = S.hp - 4;
    matt_pairs(S.rc, [&](int r, int h, int li) {
        const int c = kMattHeadDim * h + 2 * li;
        lds_f kv = A.kv + r * A.cp + c;
        lds_cf q = A.Q + r * S.hp + c;
        lds_cf da = A.dattn + r * S.hp + c;
        lds_f dq = A.dQ + r * S.hp + c;
        const float p = expf(A.sc[r * A.sp + 4 * jj + h] - A.ml[r * 8 + h]) / A.ml[r * 8 + 4 + h];
        const float vp0 = kv[H], vp1 = kv[H + 1];
        const float t = sum16(dot2(da[0], leaky(vp0), da[1], leaky(vp1)));
        const float ds = p * (t - A.Dh[r * 4 + h]) * kMattScale;
        dq[0] += ds * kv[0];
        dq[1] += ds * kv[1];
        kv[0] = ds * q[0];
        kv[1] = ds * q[1];
        kv[H] = p * da[0] * (vp0 > 0.f ? 1.f : kLeakySlope);
        kv[H + 1] = p * da[1] * (vp1 > 0.f ? 1.f : kLeakySlope);
    });
}

// V_i of the chunk's rows into column 0 of outb.  col0: the record column of agent 0's observation block (the blocks are contiguous, in
// agent order and equally wide).  Leaves for the backward: e_i and fc_out's output in xcat, Q, the normalised attn, the scores with m and
// l, the (normalised) hidden row in h2 with its rstd and mask.  Ends with a barrier.
__device__ __forceinline__ void matt_fwd(const EngineDesc& D, const NetDesc& N, g_cf thC, g_cf thA, const Lds& S, const MappoLds& X, const MattLds& A,
                                         const MattRows& R, int col0, int i) {
    const int n = D.n_agents, O = D.rec.obs_dim[0], kpad = N.L[MATT_ENC].k_pad, H = S.hp - 4, rc = S.rc;
    const bool fnorm = D.feature_norm != 0;
    if (fnorm) {
        matt_row_stats(A, R, col0, n * O, rc);
        FRL_PHASE(S);
    }
    matt_load_seg(S, A, R, col0 + i * O, O, kpad, fnorm);
    FRL_PHASE(S);
    linear_fwd(N.L[MATT_ENC], thC, S.xin, S.xp, A.xcat, A.cp, ACT_NONE, rc);
    FRL_PHASE(S);
    linear_fwd(N.L[MATT_Q], thA, A.xcat, A.cp, A.Q, S.hp, ACT_NONE, rc);
    for (int j = 0, jj = 0; j < n; ++j) {
        if (j == i) continue;
        matt_load_seg(S, A, R, col0 + j * O, O, kpad, fnorm);
        FRL_PHASE(S);
        linear_fwd(N.L[MATT_ENC], thC, S.xin, S.xp, S.h1, S.hp, ACT_NONE, rc);
        FRL_PHASE(S);
        linear_fwd(N.L[MATT_KV], thA, S.h1, S.hp, A.kv, A.cp, ACT_NONE, rc);
        FRL_PHASE(S);
        matt_attend(S, A, jj++);
        FRL_PHASE(S);
    }
    matt_pairs(rc, [&](int r, int h, int li) {
        lds_f at = A.attn + r * S.hp + kMattHeadDim * h + 2 * li;
        const float l = A.ml[r * 8 + 4 + h];
        at[0] /= l;
        at[1] /= l;
    });
    FRL_PHASE(S);
    linear_fwd(N.L[MATT_O], thA, A.attn, S.hp, A.xcat + H, A.cp, ACT_NONE, rc);
    FRL_PHASE(S);
    linear_fwd(N.L[MATT_L1], thC, A.xcat, A.cp, S.h2, S.hp, ACT_RELU, rc);
    FRL_PHASE(S);
    if (D.layer_norm) {
        ln_rows(S.h2, S.hp, H, rc, X.rstd, X.mask);
        FRL_PHASE(S);
    }
    linear_fwd(N.L[MATT_L3], thC, S.h2, S.hp, S.outb, S.op, ACT_NONE, rc);
    FRL_PHASE(S);
}

// Backward of the same: d loss / d V in column 0 of outb (zero in its pad columns and in invalid rows), all six layers' gradients to G
// (gs: GS_STORE for a step's first chunk, GS_ADD after it).  Ends with a barrier.
__device__ __forceinline__ void matt_bwd(const EngineDesc& D, const NetDesc& N, g_cf thC, g_cf thA, g_f G, const Lds& S, const MappoLds& X,
                                         const MattLds& A, const MattRows& R, int col0, int i, int gs) {
    const int n = D.n_agents, O = D.rec.obs_dim[0], kpad = N.L[MATT_ENC].k_pad, H = S.hp - 4, rc = S.rc, ht = H / 16;
    const bool fnorm = D.feature_norm != 0;
    lds_f dl = S.h2;                                    // l1's delta
    linear_bwd_dw(N.L[MATT_L3], G, S.outb, S.op, S.h2, S.hp, rc, gs);
    if (D.layer_norm) {
        dl = X.dbuf;
        linear_bwd_dx(N.L[MATT_L3], thC, S.outb, S.op, X.dbuf, S.hp, ACT_NONE, rc, 0, ht);
        FRL_PHASE(S);
        ln_bwd_rows(X.dbuf, S.h2, S.hp, H, rc, X.rstd, X.mask);
    } else {
        FRL_PHASE(S);
        linear_bwd_dx(N.L[MATT_L3], thC, S.outb, S.op, S.h2, S.hp, ACT_RELU, rc, 0, ht);
    }
    FRL_PHASE(S);
    linear_bwd_dw(N.L[MATT_L1], G, dl, S.hp, A.xcat, A.cp, rc, gs);
    linear_bwd_dx(N.L[MATT_L1], thC, dl, S.hp, A.dx, A.cp, ACT_NONE, rc, 0, 2 * ht);      // [d e_i | d att]
    FRL_PHASE(S);
    linear_bwd_dw(N.L[MATT_O], G, A.dx + H, A.cp, A.attn, S.hp, rc, gs);
    linear_bwd_dx(N.L[MATT_O], thA, A.dx + H, A.cp, A.dattn, S.hp, ACT_NONE, rc, 0, ht);
    FRL_PHASE(S);
    matt_pairs(rc, [&](int r, int h, int li) {
        const int c = kMattHeadDim * h + 2 * li;
        lds_cf da = A.dattn + r * S.hp + c;
        lds_cf at = A.attn + r * S.hp + c;
        const float d = sum16(dot2(da[0], at[0], da[1], at[1]));
        if (li == 0) A.Dh[r * 4 + h] = d;
        A.dQ[r * S.hp + c] = 0.f;
        A.dQ[r * S.hp + c + 1] = 0.f;
    });
    for (int j = 0, jj = 0; j < n; ++j) {
        if (j == i) continue;
        const int gsj = jj == 0 ? gs : GS_ADD;
        matt_load_seg(S, A, R, col0 + j * O, O, kpad, fnorm);
        FRL_PHASE(S);
        linear_fwd(N.L[MATT_ENC], thC, S.xin, S.xp, S.h1, S.hp, ACT_NONE, rc);
        FRL_PHASE(S);
        linear_fwd(N.L[MATT_KV], thA, S.h1, S.hp, A.kv, A.cp, ACT_NONE, rc);
        FRL_PHASE(S);
        matt_attend_bwd(S, A, jj++);
        FRL_PHASE(S);
        linear_bwd_dw(N.L[MATT_KV], G, A.kv, A.cp, S.h1, S.hp, rc, gsj);
        linear_bwd_dx(N.L[MATT_KV], thA, A.kv, A.cp, A.dej, S.hp, ACT_NONE, rc, 0, ht);
        FRL_PHASE(S);
        linear_bwd_dw(N.L[MATT_ENC], G, A.dej, S.hp, S.xin, S.xp, rc, gsj);
        FRL_PHASE(S);
    }
    matt_load_seg(S, A, R, col0 + i * O, O, kpad, fnorm);
    linear_bwd_dw(N.L[MATT_Q], G, A.dQ, S.hp, A.xcat, A.cp, rc, gs);
    linear_bwd_dx(N.L[MATT_Q], thA, A.dQ, S.hp, A.dej, S.hp, ACT_NONE, rc, 0, ht);
    FRL_PHASE(S);
    for (int e = threadIdx.x; e < rc * H; e += kWG) {                                      // d e_i = l1's part + Wq^T d Q
        const int r = e / H, c = e - r * H;
        A.dej[r * S.hp + c] += A.dx[r * A.cp + c];
    }
    FRL_PHASE(S);
    linear_bwd_dw(N.L[MATT_ENC], G, A.dej, S.hp, S.xin, S.xp, rc, GS_ADD);
    FRL_PHASE(S);
}

// clip_grad_norm_ over the critic's 12 tensors, then Adam with its own moments: the first three layers step thC (its own net), the
// attention layers thA (net 1).  query and key have no bias: their bias gradients are cleared first, so the slots stay zero.  Returns
// the norm before clipping.
__device__ __forceinline__ float matt_adam(const NetDesc& N, g_f thC, g_f thA, g_f m, g_f v, g_f G, float lr, float eps, float b1, float b2,
                                           float clip_norm, int t_new, lds_f red) {
    for (int c = threadIdx.x; c < kMattHidden; c += kWG) {
        G[N.L[MATT_Q].b_off + c] = 0.f;
        G[N.L[MATT_KV].b_off + c] = 0.f;
    }
    __syncthreads();
    const int n4 = N.size >> 2, split4 = N.L[MATT_Q].w_off >> 2;
    float ss = 0.f;
    for (int k = threadIdx.x; k < n4; k += kWG) {
        const f32x4 x = ld4((g_cf)G + 4 * k);
        ss += (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
    }
    const float total = sqrtf(block_sum(ss, red));
    const AdamCoef c = adam_coef(total, clip_norm, t_new, lr, b1, b2, eps, 0.f, 0.f);
    for (int k = threadIdx.x; k < n4; k += kWG) {
        g_f th = (k < split4 ? thC : thA) + 4 * k;
        f32x4 mi = ld4((g_cf)m + 4 * k), vi = ld4((g_cf)v + 4 * k);
        const f32x4 t = adam_exact4(ld4((g_cf)th), ld4((g_cf)G + 4 * k) * c.coef, mi, vi, c.w1, c.w2, b2, c.bc2s, eps, c.step);
        st4(m + 4 * k, mi);
        st4(v + 4 * k, vi);
        st4(th, t);
    }
    return total;
}

// ---- all K_epochs x minibatch steps of critic i of learner p by the calling workgroup (MAPPO_attention.py:378-400), as mappo_steps
// runs a plain critic's: v_s repeated over all n target columns, the loss kinds of onpolicy.hpp's value_row
__device__ __forceinline__ void matt_critic_steps(const EngineDesc& D, const MappoArgs& a, const Lds& S, const MappoLds& X, const MattLds& A, int p, int i,
                                                  float* norm_trace) {
    const int n = D.n_agents, u = p * n + i, net = 2 * i + 1;
    const int T = a.horizon, mb = a.minibatch, rc = D.rc;
    const NetDesc& N = D.net[net];
    const RecordDesc& R = D.rec;
    const size_t off = (size_t)p * D.learner_stride + D.net_off[net];
    g_f thC = as_global(D.theta + off);
    g_f thA = as_global(D.theta + (size_t)p * D.learner_stride + D.net_off[1]);
    g_f G = as_global(D.grad + off);
    g_cf ring = as_global(D.replay + (size_t)p * D.capacity * R.stride);
    g_cf vt = as_global(a.vtarget + (size_t)p * T * n);
    const int npad = N.L[MATT_L3].n_pad;
    int* steps = D.steps + (size_t)p * (kMaxNets + 1);
    int t_adam = steps[net];
    const int n_mb = (T + mb - 1) / mb;
    float* trace = a.trace + (size_t)u * a.k_epochs * n_mb * 2;
    LearnArgs la = {};
    la.huber = a.huber;
    la.huber_delta = a.huber_delta;
    float last = 0.f;
    for (int k = 0; k < a.k_epochs; ++k) {
        g_ci perm = as_global_i(a.perm + ((size_t)u * a.k_epochs + k) * T);
        for (int s = 0; s < T; s += mb) {
            const int m = min(mb, T - s);
            const float invmn = 1.f / (float)(m * n);
            const int j_tr = k * n_mb + s / mb;
            float lossp = 0.f;
            for (int r0 = 0; r0 < m; r0 += rc) {
                const MattRows rows = {ring, perm + s + r0, 0, R.stride, min(rc, m - r0)};
                matt_fwd(D, N, thC, thA, S, X, A, rows, R.obs_off[0], i);
                if (threadIdx.x < rc) {
                    const int r = threadIdx.x;
                    float d = 0.f;
                    if (r < rows.nv) d = value_row(la, S.outb[r * S.op], vt + (size_t)rows.idx[r] * n, 0, n, lossp) * invmn;
                    S.outb[r * S.op] = d;
                    for (int c = 1; c < npad; ++c) S.outb[r * S.op + c] = 0.f;
                }
                __syncthreads();
                matt_bwd(D, N, thC, thA, G, S, X, A, rows, R.obs_off[0], i, r0 == 0 ? GS_STORE : GS_ADD);
            }
            const float loss = block_sum(lossp, S.red) * invmn;
            __syncthreads();
            ++t_adam;
            const float gnorm = matt_adam(N, thC, thA, as_global(D.m + off), as_global(D.v + off), G, a.critic_lr, a.adam_eps, a.beta1, a.beta2, a.clip_norm,
                                          t_adam, S.red);
            __syncthreads();
            if (threadIdx.x == 0) {
                trace[2 * j_tr + 1] = loss;
                if (norm_trace) norm_trace[(size_t)u * a.k_epochs * n_mb + j_tr] = gnorm;
            }
            last = loss;
        }
    }
    if (threadIdx.x == 0) {
        steps[net] = t_adam;
        D.stats[(size_t)u * ST_COUNT + ST_CRITIC_LOSS] = last;
    }
}

}  // namespace frl
