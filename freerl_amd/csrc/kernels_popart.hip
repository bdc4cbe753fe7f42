// PopArt DDPG (DDPG_file/DDPG_simple_with_tricks.py:95-292 with trick['popart']) on the row-chunk skeleton: kernels_cem_gd3pg.hip's
// critic-then-actor shape with ReLU nets and an adaptive target normaliser between the critic and every place its output is read.
// Launch chain (frl_api_popart.inc):
//     [draw_kernel] -> popart_target_kernel -> popart_critic_kernel -> popart_step_kernel (critic + upper layer)
//                   -> popart_actor_kernel -> popart_step_kernel (actor)
// Net 0 is the actor (obs -> H ReLU -> H ReLU -> A tanh), net 1 PopArt's lower layers ([obs | act] -> H ReLU -> H ReLU -> 1).  The upper
// layer Linear(1, 1) {W, b}, the statistics {sigma, mu, nu} and the upper layer's Adam state are ten floats of the learner's block in
// EngineDesc::popart (rowchunk_layout.h).
// The critic's delta e = W h + b - (y - mu') / sigma' needs mu', sigma' and the popped W, b, which are functions of mean(y) and mean(y^2)
// over the WHOLE batch: hence a target launch ahead of the critic launch.  Its workgroups park y in HBM and leave sum y, sum y^2 of
// their rows (accumulated in double) in their part slots; every workgroup of the critic launch adds the slots in slice order and derives
// the same bits of the step (popart_next, device/popart.hpp) into registers.  The alternatives to the second launch are a grid-wide wait
// inside one launch — every workgroup resident, as kernels_solo.hip has to arrange — or, by linearity of the backward in its seed,
// three backward passes on seeds h, 1 and y combined afterwards; the launch costs a few microseconds and is the cheapest of the three.
// popart_step_kernel is reduce + clip + Adam + soft update as cem_step_kernel; behind the critic's step one lane owns the upper layer:
// pop, the clip over its own two gradients, its Adam, and the write-back of W, b, sigma, mu, nu — the only writer of those five.
// DDPG's ac_actor_kernel is NOT reused for the actor launch: its critic seed -1/B is a constant of the launch, this one's -sigma' W / B is
// a learner's, read from the block, and threading it through would put a load and a branch into the DDPG / TD3 / SAC kernel.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "device/net.hpp"
#include "device/act_common.hpp"
#include "device/popart.hpp"
#include "device/update_common.hpp"

namespace frl {

// ------------------------------------------------------------------------------------- target
// y = r + gamma (1 - done) (sigma (W critic_target(s', actor_target(s')) + b) + mu) (:258-265): the OLD statistics and the ONLINE upper
// layer, read once per workgroup.  The target action goes straight into the critic's input row, as in cem_critic_kernel.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void popart_target_kernel(const EngineDesc* __restrict__ Dp, PopartArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[POP_ACTOR];
    const NetDesc& NC = D.net[POP_CRITIC];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.rows;
    const RowWalk W = U.walk(B);
    g_cf tgA = U.target(POP_ACTOR);
    g_cf tgC = U.target(POP_CRITIC);
    g_cf ring = U.ring();
    const int O = R.obs_dim[0], A = R.act_dim[0];
    const int kc0 = NC.L[0].k_pad;
    const float* hd = popart_head(D, U.p);
    const float uW = hd[POP_W], ub = hd[POP_B], sigma = hd[POP_SIGMA], mu = hd[POP_MU];

    double syp = 0.0, sy2p = 0.0;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup
    const UnitChunk c = W.chunk(ck);
    const int nv = c.nv;
    g_ci idx = c.idx;
    g_f ypark = popart_y_rows(U, c.r0);
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.nobs_off[0], O, 0);
    zero_cols(S.xin, S.xp, rc, O, kc0);      // (the critic's first layer is the wider one: the actor's reads zeros past s')
    FRL_PHASE(S);
    mlp_fwd_rows(NA, 0, NA.n_layers, tgA, S, ACT_TANH, [&](int r) {
        for (int k = 0; k < A; ++k) S.xin[r * S.xp + O + k] = S.outb[r * S.op + k];
    });
    mlp_fwd_rows(NC, 0, NC.n_layers, tgC, S, ACT_NONE, [&](int r) {
        if (r >= nv) return;
        g_cf rec = ring + (size_t)idx[r] * R.stride;
        const float q = sigma * (uW * S.outb[r * S.op] + ub) + mu;
        const float y = rec[R.rew_off] + a.gamma * q * (1.f - rec[R.done_off]);
        ypark[r] = y;
        syp += (double)y;
        sy2p += (double)y * (double)y;
    });
    }
    const double sy = popart_block_sum(syp, S.red), sy2 = popart_block_sum(sy2p, S.red);
    if (threadIdx.x == 0) {
        double* pd = (double*)popart_part(U);
        pd[POP_PART_SY / 2] = sy;
        pd[POP_PART_SY2 / 2] = sy2;
    }
}

// ------------------------------------------------------------------------------------- critic
// PopArt.forward (:170-181) up to the backward: loss = mean (W h + b - (y - mu') / sigma')^2 with h = critic(s, a) and the popped W, b.
// The seed into the lower layers is dloss/dh = 2 e W / B; the upper layer's own gradients dW = sum 2 e h / B, db = sum 2 e / B go to
// the part slot with the loss.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void popart_critic_kernel(const EngineDesc* __restrict__ Dp, PopartArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const RecordDesc& R = D.rec;
    const NetDesc& NC = D.net[POP_CRITIC];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.rows;
    const RowWalk W = U.walk(B);
    g_cf thC = U.theta(POP_CRITIC);
    g_f slab = U.slab(POP_CRITIC);
    g_cf ring = U.ring();
    const int O = R.obs_dim[0], A = R.act_dim[0];
    const int kc0 = NC.L[0].k_pad, npad = NC.L[NC.n_layers - 1].n_pad;
    const PopartStep n = popart_next(D, U.p, ns, B, a.beta);      // (registers only: popart_step_kernel writes the block)
    const float uW = n.W, ub = n.b, mu = n.mu, sigma = n.sigma;
    const float k2 = 2.f / (float)B;

    float lossp = 0.f, dWp = 0.f, dbp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, nv = c.nv;
    g_cf ypark = popart_y_rows(U, c.r0);
    // ---- critic on [s | a] (adjacent in a record), the normalised TD delta, backward
    gather_cols(S.xin, S.xp, rc, nv, c.idx, ring, R.stride, R.obs_off[0], O + A, 0);
    zero_cols(S.xin, S.xp, rc, O + A, kc0);
    FRL_PHASE(S);
    mlp_fwd_rows(NC, 0, NC.n_layers, thC, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        float d = 0.f;
        if (r < nv) {
            const float h = o[0];
            const float e = (uW * h + ub) - (ypark[r] - mu) / sigma;
            lossp += e * e;
            dWp += k2 * e * h;
            dbp += k2 * e;
            d = k2 * e * uW;
        }
        o[0] = d;
        for (int k = 1; k < npad; ++k) o[k] = 0.f;
    });
    mlp_bwd(NC, 0, NC.n_layers, thC, slab, S, gs, false, 0, 0);
    }
    const float ls = block_sum(lossp, S.red), dW = block_sum(dWp, S.red), db = block_sum(dbp, S.red);
    if (threadIdx.x == 0) {
        float* pt = popart_part(U);
        pt[POP_PART_LOSS] = ls;
        pt[POP_PART_DW] = dW;
        pt[POP_PART_DB] = db;
    }
}

// -------------------------------------------------------------------------------------- actor
// loss = -mean (sigma' (W critic(s, actor(s)) + b) + mu') (:274-279) through the lower critic and the upper layer just stepped: the critic's
// constant head delta is -sigma' W / B, a dX-only backward to the action's column tiles, then the actor's backward — cem_actor_kernel's
// shape with one actor and no penalty.  The part slot gets sum -h; popart_step_kernel forms the loss from it.
__global__ __launch_bounds__(256, FRL_GRAD_WGS) void popart_actor_kernel(const EngineDesc* __restrict__ Dp, PopartArgs a, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const EngineDesc& D = *Dp;
    const RowUnit U = learner_unit(D, ns, a.p0, a.p_count);
    if (U.none) return;
    const RecordDesc& R = D.rec;
    const NetDesc& NA = D.net[POP_ACTOR];
    const NetDesc& NC = D.net[POP_CRITIC];
    const Lds S = carve(D, smem);
    const int rc = D.rc, B = a.rows;
    const RowWalk W = U.walk(B);
    g_cf thA = U.theta(POP_ACTOR);
    g_cf thC = U.theta(POP_CRITIC);
    g_f slab = U.slab(POP_ACTOR);
    g_cf ring = U.ring();
    const int O = R.obs_dim[0], A = R.act_dim[0];
    const int ka0 = NA.L[0].k_pad, kc0 = NC.L[0].k_pad;
    const int ncpad = NC.L[NC.n_layers - 1].n_pad, napad = NA.L[NA.n_layers - 1].n_pad;
    const int ct0 = O / 16, ct1 = (O + A + 15) / 16;            // the action's column tiles of the critic's input
    const float* hd = popart_head(D, U.p);
    const float dq = -(hd[POP_SIGMA] * hd[POP_W]) / (float)B;
    FRL_GLB f32x4* spill = U.spill();

    float alossp = 0.f;
    for (int ck = W.cr.c0; ck < W.cr.c1; ++ck) {       // the row chunks of this workgroup, their gradients summed in its slab
    const UnitChunk c = W.chunk(ck);
    const int gs = c.gs, nv = c.nv;
    g_ci idx = c.idx;
    // ---- a = actor(s): kept in abuf for tanh', and written into the critic's input row
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);
    zero_cols(S.xin, S.xp, rc, O, kc0);
    FRL_PHASE(S);
    mlp_fwd_rows(NA, 0, NA.n_layers, thA, S, ACT_TANH, [&](int r) {
        for (int k = 0; k < A; ++k) {
            const float av = S.outb[r * S.op + k];
            S.abuf[r * S.ap + k] = av;
            S.xin[r * S.xp + O + k] = av;
        }
    }, [&]() { park_hidden(S, spill); });
    // ---- the stepped critic on [s | a]: h into the loss sum, the constant head delta, dX into the action column tiles
    mlp_fwd_rows(NC, 0, NC.n_layers, thC, S, ACT_NONE, [&](int r) {
        lds_f o = S.outb + r * S.op;
        const bool live = r < nv;
        if (live) alossp -= o[0];
        o[0] = live ? dq : 0.f;
        for (int k = 1; k < ncpad; ++k) o[k] = 0.f;
    });
    mlp_bwd(NC, 0, NC.n_layers, thC, nullptr, S, GS_ADD, true, ct0, ct1);
    for (int e = threadIdx.x; e < rc * A; e += kWG) {
        const int r = e / A, k = e - r * A;
        S.dabuf[r * S.ap + k] = S.xin[r * S.xp + O + k];
    }
    FRL_PHASE(S);
    // ---- the actor's activations back from HBM (same thread, same addresses as the spill), its input back in xin
    restore_hidden(S, spill);
    gather_cols(S.xin, S.xp, rc, nv, idx, ring, R.stride, R.obs_off[0], O, 0);      // (the critic's dX landed on xin)
    zero_cols(S.xin, S.xp, rc, O, ka0);
    // the head delta in the same phase: it reads dabuf / abuf and writes outb, none of which the reload above touches
    for (int e = threadIdx.x; e < rc * napad; e += kWG) {
        const int r = e / napad, k = e - r * napad;
        S.outb[r * S.op + k] = (r < nv && k < A) ? tanh_delta(S.dabuf[r * S.ap + k], S.abuf[r * S.ap + k]) : 0.f;
    }
    FRL_PHASE(S);
    mlp_bwd(NA, 0, NA.n_layers, thA, slab, S, gs, false, 0, 0);
    }
    const float la = block_sum(alossp, S.red);
    if (threadIdx.x == 0) popart_part(U)[POP_PART_ACTOR] = la;
}

// ------------------------------------------------------------------------------- reduce + step
// One workgroup per learner: the slices' slabs summed in slice order into the learner's grad block, then clip_grad_norm_(0.5) + torch-order
// Adam + the soft update of the net's target (adam_net) and the step count.  stage 0: the lower critic, then thread 0 alone on the
// upper layer and the statistics (:135-146, :165-166); stage 1: the actor, and the call's outputs.
__global__ __launch_bounds__(256) void popart_step_kernel(const EngineDesc* __restrict__ Dp, PopartArgs a, int ns) {
    __shared__ float red_s[8];
    const EngineDesc& D = *Dp;
    const int p = a.p0 + blockIdx.x, net = a.stage == 0 ? (int)POP_CRITIC : (int)POP_ACTOR;
    const NetDesc& N = D.net[net];
    const size_t off = (size_t)p * D.learner_stride + D.net_off[net];
    const int n4 = N.size / 4;                                          // (a net's size is a multiple of 32 floats)
    FRL_GLB f32x4* g = (FRL_GLB f32x4*)(D.grad + off);
    const FRL_GLB f32x4* slab = (const FRL_GLB f32x4*)(D.slab + slab_offset(D, p, 0, net));      // slice 0; slice k lies k learner strides further
    const size_t ls4 = (size_t)D.learner_stride / 4;
    for (int i = threadIdx.x; i < n4; i += kWG) {
        f32x4 s = slab[i];
        for (int k = 1; k < ns; ++k) s += slab[(size_t)k * ls4 + i];
        g[i] = s;
    }
    __syncthreads();
    int* steps = D.steps + (size_t)p * (kMaxNets + 1);
    const int t = steps[net] + 1;
    const float lr = a.stage == 0 ? a.critic_lr : a.actor_lr;
    const float total = adam_net(N.size, as_global(D.theta + off), as_global(D.m + off), as_global(D.v + off), as_global((const float*)(D.grad + off)),
                                 as_global(D.target + off), lr, 1e-8f, 0.9f, 0.999f, 0.f, 0.5f, t, a.tau, (lds_f)red_s);
    if (threadIdx.x != 0) return;
    steps[net] = t;
    float* hd = popart_head(D, p);
    float* out = D.popart_out + (size_t)p * kPopartOut;
    float* st = D.stats + (size_t)p * ST_COUNT;
    float sums[kPopartPart - POP_PART_LOSS] = {0.f, 0.f, 0.f, 0.f};      // loss, dW, db, sum -h: the slices' partials in slice order
    for (int k = 0; k < ns; ++k) {
        const float* pt = D.popart + popart_part_offset(D, p, k);
        for (int j = (a.stage == 0 ? 0 : 3); j < (a.stage == 0 ? 3 : 4); ++j) sums[j] += pt[POP_PART_LOSS + j];
    }
    if (a.stage == 0) {
        const PopartStep n = popart_next(D, p, ns, a.rows, a.beta);
        float uW = n.W, ub = n.b;
        int* ustep = (int*)(hd + POP_STEP);
        const int ut = *ustep + 1;
        const float unorm = popart_upper_step(hd, uW, ub, sums[1], sums[2], a.upper_lr, ut);
        *ustep = ut;
        hd[POP_W] = uW; hd[POP_B] = ub; hd[POP_SIGMA] = n.sigma; hd[POP_MU] = n.mu; hd[POP_NU] = n.nu;
        out[POP_OUT_CRITIC_LOSS] = st[ST_CRITIC_LOSS] = sums[0] / (float)a.rows;
        out[POP_OUT_LOWER_NORM] = st[ST_CRITIC_GNORM] = total;
        out[POP_OUT_UPPER_NORM] = unorm;
        out[POP_OUT_SIGMA] = n.sigma;
        out[POP_OUT_MU] = n.mu;
        out[POP_OUT_ROWS] = n.guard ? -(float)a.rows : (float)a.rows;
        return;
    }
    // -mean(sigma (W h + b) + mu) with what stage 0 left: mean h = -sums[3] / B
    const float hbar = -sums[3] / (float)a.rows;
    out[POP_OUT_ACTOR_LOSS] = st[ST_ACTOR_LOSS] = -(hd[POP_SIGMA] * (hd[POP_W] * hbar + hd[POP_B]) + hd[POP_MU]);
    out[POP_OUT_ACTOR_NORM] = st[ST_ACTOR_GNORM] = total;
}

}  // namespace frl
