// REINFORCE (REINFORCE_file/REINFORCE.py:104-127): one policy-gradient step per learner on the steps its ring has stored since the
// last call — a contiguous, variable-length batch, rows 0..n-1 in time order.  Launch chain (frl_api_reinforce.inc):
//     reinforce_returns_kernel -> reinforce_grad_kernel -> reduce + Adam (kernels_update.hip, AdamArgs::ragged)
// Every learner brings its own row count EngineDesc::ep_n[p]; a learner with none sits the call out: its workgroups of all three
// launches return before they read or write anything of it.
#include <hip/hip_runtime.h>

#include "device/gae.hpp"
#include "device/lane.hpp"
#include "device/onpolicy.hpp"
#include "device/update_common.hpp"
#include "kernels.h"

namespace frl {

// ------------------------------------------------------------------------------------ returns
// G_t = r_t + gamma G_{t+1} (1 - done_t) is the affine map G -> b + a G with a = gamma (1 - done_t), b = r_t; a run of steps is the
// composition of its maps: gae.hpp's AffineD, compose(f, g) = f after g, where g belongs to the LATER steps (the scan runs backwards
// in time).

template <int OFF>
__device__ __forceinline__ double lane_xor_d(double v) {
    const int lo = lane_xor<OFF>(__double2loint(v)), hi = lane_xor<OFF>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// One butterfly step of the wave's reverse scan: before it `scan` covers the lane's steps up to the end of its aligned block of OFF
// lanes and `tot` the whole block; afterwards the same for blocks of 2 OFF lanes.  Both halves form `tot` from the same two operands
// in the same order, so every lane of a block holds the same bits.
template <int OFF>
__device__ __forceinline__ void rscan_step(AffineD& scan, AffineD& tot) {
    const AffineD o{lane_xor_d<OFF>(tot.a), lane_xor_d<OFF>(tot.b)};
    if (threadIdx.x & OFF) {
        tot = compose(o, tot);
    } else {
        scan = compose(scan, o);
        tot = compose(tot, o);
    }
}
__device__ __forceinline__ double wave_sum_d(double v) {
    v += lane_xor_d<32>(v); v += lane_xor_d<16>(v); v += lane_xor_d<8>(v);
    v += lane_xor_d<4>(v); v += lane_xor_d<2>(v); v += lane_xor_d<1>(v);
    return v;
}
// the four waves' sums added in wave order: the same bits in every thread and every run
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup per learner.  Returns in float64 like the reference's Python floats (:108-112), cast to float32 once (:114); then
// (G - mean) / (std + 1e-8) with torch.std's n - 1 (:117) into isw[p][0..n).  Lane l owns the contiguous steps [l seg, (l + 1) seg):
// pass 1 composes their maps, the lanes' maps are scanned backwards (butterfly in the wave, the four waves' totals through LDS),
// which gives every lane the return that enters its segment from the right; pass 2 walks the segment once more with the
// reference's own expression and writes the rows.  A lane reads back only rows it wrote itself.  The mean and the squared
// deviations are summed in float64 per lane and combined in a fixed order: two runs give the same bits, and equal returns give a
// mean equal to them, so that their normalised value is exactly zero as it is in the reference.
__global__ __launch_bounds__(256) void reinforce_returns_kernel(const EngineDesc* __restrict__ Dp, double gamma) {
    __shared__ double wave_a[4], wave_b[4], red[4];
    __shared__ double g_in[kWG + 1];
    const EngineDesc& D = *Dp;
    const int p = blockIdx.x, n = D.ep_n[p];
    if (n <= 0) return;
    const RecordDesc& R = D.rec;
    const float* ring = D.replay + (size_t)p * D.capacity * R.stride;
    float* w = D.isw + (size_t)p * D.batch_max;
    const int tid = threadIdx.x, seg = (n + kWG - 1) / kWG;
    const int t0 = min(tid * seg, n), t1 = min(t0 + seg, n);

    AffineD f{1.0, 0.0};
    for (int t = t1 - 1; t >= t0; --t) {
        const float* rec = ring + (size_t)t * R.stride;
        const double a = gamma * (1.0 - (double)rec[R.done_off]);
        f = AffineD{a * f.a, (double)rec[R.rew_off] + a * f.b};
    }
    AffineD scan = f, tot = f;
    rscan_step<1>(scan, tot); rscan_step<2>(scan, tot); rscan_step<4>(scan, tot);
    rscan_step<8>(scan, tot); rscan_step<16>(scan, tot); rscan_step<32>(scan, tot);
    if ((tid & 63) == 0) { wave_a[tid >> 6] = tot.a; wave_b[tid >> 6] = tot.b; }
    __syncthreads();
    for (int wv = (tid >> 6) + 1; wv < kWG / 64; ++wv) scan = compose(scan, AffineD{wave_a[wv], wave_b[wv]});
    g_in[tid] = scan.b;                            // the return at the lane's first step: nothing follows the last step (G = 0)
    if (tid == 0) g_in[kWG] = 0.0;
    __syncthreads();

    double G = g_in[tid + 1], sum = 0.0;
    for (int t = t1 - 1; t >= t0; --t) {
        const float* rec = ring + (size_t)t * R.stride;
        // rewards[t] + gamma * G * (1 - dones[t]), rounded product by product as Python does (no fused multiply-add)
        G = __dadd_rn((double)rec[R.rew_off], __dmul_rn(__dmul_rn(gamma, G), 1.0 - (double)rec[R.done_off]));
        const float g32 = (float)G;
        w[t] = g32;
        sum += (double)g32;
    }
    const float mean = (float)(block_sum_d(sum, red) / (double)n);
    double ss = 0.0;
    for (int t = t0; t < t1; ++t) {
        const float d = w[t] - mean;
        ss += (double)d * (double)d;
    }
    const float sd = sqrtf((float)(block_sum_d(ss, red) / (double)(n - 1)));
    const float denom = sd + 1e-8f;
    for (int t = t0; t < t1; ++t) w[t] = (w[t] - mean) / denom;
}

// --------------------------------------------------------------------------------------- grad
// loss = sum_t -log pi(a_t | s_t) g_t (:119-121, a sum) on the row-chunk skeleton: a workgroup's chunks are consecutive ring rows.
// Categorical(probs = softmax(z)) (:82-85) renormalises the probabilities and takes log(clamp(q, eps, 1 - eps)), so the head delta
// is g_t (q - onehot(a_t)), and zero for a row whose q[a_t] lies outside [eps, 1 - eps] (the clamp passes no gradient there).
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void reinforce_grad_kernel(const EngineDesc* __restrict__ Dp, int p0, int p_count, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, p0, p_count);
    if (U.none) return;
    const int p = U.p;
    const int n = D.ep_n[p];
    const RowWalk W = U.walk(n);
    if (W.cr.c0 >= W.cr.c1) return;                    // the learner sits out, or its rows end before this workgroup's chunks
    const NetDesc& N = D.net[0];
    const RecordDesc& R = D.rec;
    const Lds S = carve(D, smem);
    const int rc = D.rc, nl = N.n_layers;
    g_cf theta = U.theta(0);
    g_f slab = U.slab(0);
    g_cf ring = U.ring();
    g_cf gw = as_global(D.isw + (size_t)p * D.batch_max);
    const int O = R.obs_dim[0], A = D.n_discrete, npad = N.L[nl - 1].n_pad, k0pad = N.L[0].k_pad;

    float lossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, r0 = c.r0, nv = c.nv;
    g_cf rows = ring + (size_t)r0 * R.stride;      // a workgroup's chunks are consecutive ring rows: no idx
    load_rows(S.xin, S.xp, rc, nv, rows, 0, R.stride, R.obs_off[0], O, k0pad);
    lds_barrier();
    mlp_fwd_rows(N, 0, nl, theta, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        const int act = (r < nv) ? (int)rows[(size_t)r * R.stride + R.act_off[0]] : -1;
        if (act >= 0 && act < A) {
            // F.softmax (max-subtracted, divided by the sum), then Categorical's probs / probs.sum(-1): onpolicy.hpp's CatRow
            CatRow q = cat_softmax(o, A);
            for (int j = 0; j < A; ++j) { o[j] = q.prob(o[j]); q.psum += o[j]; }
            const float g = gw[r0 + r];
            const float qa = o[act] / q.psum;
            const bool open = qa >= kProbEps && qa <= 1.f - kProbEps;
            lossp -= (float)log((double)q.clamped(o[act])) * g;      // correctly rounded, as select_action records it
            for (int c = 0; c < npad; ++c) o[c] = (open && c < A) ? g * (o[c] / q.psum - (c == act ? 1.f : 0.f)) : 0.f;
        } else {
            for (int c = 0; c < npad; ++c) o[c] = 0.f;
        }
    });
    mlp_bwd(N, 0, nl, theta, slab, S, gs, false, 0, 0);
    }
    store_loss_part(U, S, lossp);
}
}  // namespace frl
