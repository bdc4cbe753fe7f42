// select_action's shared device code: the action / exploration rules behind a policy's head outputs (act_epilogue) and the
// register-chained forward of the fragment-image engines in front of it (act_frag_body) — kernels_act.hip's two kernels, and the
// tail of kernels_solo.hip's launches in the rollout loop (the next step's select_action folded into the update's launch).
#pragma once
#include "c51.hpp"
#include "onpolicy.hpp"
#include "chain_net.hpp"
#include "special.hpp"

namespace frl {

// ---- The Beta actor's draw (Actor_Beta, PPO_with_tricks.py:120-151,243-247): act_epilogue<true>, ACTM_PPO_SAMPLE on a beta_actor engine.
constexpr int kBetaTries = 16;                                                  // attempts per gamma variate, a bound and the draws' address pitch
constexpr unsigned kStreamGammaA = 0x9400u, kStreamGammaB = 0x9500u;      // Philox streams of Ga and Gb, next to 0x9100 / 0x9200 / 0x9300 below

// G ~ Gamma(shape, 1) by Marsaglia-Tsang (2000): d = shape - 1/3, c = 1 / sqrt(9 d); with n ~ N(0,1), u ~ U(0,1] and v = (1 + c n)^3
// accept d v when v > 0 and ln u < n^2 / 2 + d - d v + d ln v.  shape = softplus(.) + 1 >= 1 here, so the method's boost for shapes
// below 1 (Gamma(shape + 1) u^(1/shape)) has no branch.  One Philox call per attempt gives n (z, w) and u (x); attempt t of element e
// reads counter word e0 + t, so a draw depends on (launch, learner, row, dimension) only.  Acceptance is >= 0.95 at shapes >= 1:
// all kBetaTries attempts fail with probability < 1e-20, and then the variate is d (the mode of d v), never a loop without end.
__device__ __forceinline__ float gamma_draw(float shape, unsigned long long counter, unsigned stream, unsigned e0, unsigned long long key) {
    const float d = shape - (1.f / 3.f), c = rsqrtf(9.f * d);
    float g = d;
    for (int t = 0; t < kBetaTries; ++t) {
        const Philox4 r = philox4x32_10(counter, stream, e0 + (unsigned)t, key);
        float n, unused;
        normal2(r, n, unused);
        const float w = 1.f + c * n, v = w * w * w;
        if (v > 0.f && logf(u01(r.x)) < 0.5f * n * n + d - d * v + d * logf(v)) { g = d * v; break; }
    }
    return g;
}

// One thread per (row, dimension c) of the 2A-wide linear head [alpha_layer ; beta_layer] in outb: alpha = softplus(z[c]) + 1 and
// beta = softplus(z[A + c]) + 1 with ppo_update_kernel's own softplus (float softplus_t, then + 1 in double), both gammas drawn by
// this thread, x = Ga / (Ga + Gb) clamped into [FLT_MIN, 1 - 2^-24] so that log(x) and log1p(-x) of the STORED float are finite
// in the update, the per-dimension log-prob in double as the update recomputes it, and the reference loop's
// action_ = clip(x * max_action, -max_action, max_action) (:529-530: it maps (0,1) into [0, max_action], kept as the script has it).
__device__ __forceinline__ void beta_sample_rows(const ActArgs& a, lds_cf outb, int op, int nv, int r0, int p, int A, unsigned long long key) {
    for (int e = threadIdx.x; e < nv * A; e += kWG) {
        const int r = e / A, c = e - r * A;
        const size_t o = ((size_t)p * a.n_rows + r0 + r) * A + c;
        const double al = (double)softplus_t(outb[r * op + c]) + 1.0, be = (double)softplus_t(outb[r * op + A + c]) + 1.0;
        const unsigned e0 = (unsigned)((r0 + r) * A + c) * (unsigned)kBetaTries;
        const float ga = gamma_draw((float)al, a.rng_counter, kStreamGammaA, e0, key);
        const float gb = gamma_draw((float)be, a.rng_counter, kStreamGammaB, e0, key);
        const float x = fminf(fmaxf(ga / (ga + gb), 1.17549435e-38f), 1.f - 5.9604645e-8f);
        a.out[o] = x;
        if (a.out_logp) a.out_logp[o] = (float)((al - 1.0) * log((double)x) + (be - 1.0) * log1p(-(double)x) - lbeta_d(al, be));
        if (a.env_out) a.env_out[o] = fminf(fmaxf(x * a.max_action, -a.max_action), a.max_action);
    }
}

// Everything after the head's output rows are in LDS (outb[row * op + column], rows r0 .. r0 + nv of learner p): the mode's
// action rule and, for the collectors, the exploration rule.  Shared by act_kernel (row-chunk forward, Wk parameters) and
// act_frag_kernel (register-chained forward, fragment-image parameters).  kBetaHead: compiled with the Beta draw above — act_kernel
// alone, the one forward a Beta engine's actor takes (PPO engines never hold fragment images); every other kernel's code is as it was.
template <bool kBetaHead = false>
__device__ __forceinline__ void act_epilogue(const EngineDesc& D, const ActArgs& a, const NetDesc& N, g_cf theta, lds_f outb, int op,
                                             int nv, int r0, int p, int nout) {
    // device-side draws of this launch: Philox keyed like draw_kernel's (seed, learner), one counter value per launch
    const unsigned long long key = D.seed + 0x9E3779B97F4A7C15ull * (p + 1);
    if constexpr (kBetaHead) {
        if (D.beta_actor && a.mode == ACTM_PPO_SAMPLE) { beta_sample_rows(a, outb, op, nv, r0, p, nout / 2, key); return; }
    }
    auto normal_at = [&](unsigned stream, unsigned e) {
        float n0, n1;
        normal2(philox4x32_10(a.rng_counter, stream, e, key), n0, n1);
        return n0;
    };
    // epsilon-greedy on the greedy index of row r (DQN.py:307-310: np.random.rand() < epsilon -> np.random.randint(action_dim))
    auto eps_greedy = [&](int row, int best, int n_act) {
        if (a.env_out && a.explore == EXPL_EPS_GREEDY) {
            const Philox4 u = philox4x32_10(a.rng_counter, 0x9000u, (unsigned)row, key);
            if (u01(u.z) <= a.epsilon) best = (int)uniform_index(u, (unsigned)n_act);      // u01 is (0,1]
        }
        return best;
    };
    if (a.mode == ACTM_ARGMAX && D.c51_atoms && D.algo == ALGO_DQN) {      // argmax_a sum_i z_i p_i(s, a) (DQN_with_tricks.py:122-130)
        const float dz = (D.c51_vmax - D.c51_vmin) / (float)(D.c51_atoms - 1);
        const int lb = c51_combine(outb, op, nv, D.n_discrete, D.c51_atoms, D.dueling != 0);
        for (int r = threadIdx.x; r < nv; r += kWG) {
            int best = 0;
            float mx = 0.f;
            for (int j = 0; j < D.n_discrete; ++j) {
                const float q = c51_q(outb + r * op + lb + j * D.c51_atoms, D.c51_atoms, D.c51_vmin, dz, nullptr);
                if (j == 0 || q > mx) { mx = q; best = j; }
            }
            best = eps_greedy(r0 + r, best, D.n_discrete);
            a.out[(size_t)p * a.n_rows + r0 + r] = (float)best;
            if (a.env_out) a.env_out[(size_t)p * a.n_rows + r0 + r] = (float)best;
        }
        return;
    }
    if (a.mode == ACTM_ARGMAX) {
        const bool duel = D.dueling && D.algo == ALGO_DQN;       // Q = V + A - mean(A) (DQN_with_tricks.py:79): head = [V ; A]
        for (int r = threadIdx.x; r < nv; r += kWG) {
            lds_cf o = outb + r * op;
            const int nq = duel ? nout - 1 : nout;
            float mean = 0.f;
            if (duel) { for (int j = 0; j < nq; ++j) mean += o[1 + j]; mean /= (float)nq; }
            int best = 0;
            float mx = duel ? (o[0] + o[1]) - mean : o[0];
            for (int j = 1; j < nq; ++j) {         // first maximum wins, like torch.argmax
                const float v = duel ? (o[0] + o[1 + j]) - mean : o[j];
                if (v > mx) { mx = v; best = j; }
            }
            best = eps_greedy(r0 + r, best, nq);
            a.out[(size_t)p * a.n_rows + r0 + r] = (float)best;
            if (a.env_out) a.env_out[(size_t)p * a.n_rows + r0 + r] = (float)best;
        }
        return;
    }
    if (a.mode == ACTM_CAT_SAMPLE) {        // PPO_with_tricks.py:249-251 (torch single-draw multinomial)
        for (int r = threadIdx.x; r < nv; r += kWG) {
            CatRow cq = cat_softmax(outb + r * op, nout);            // psum: added up in the draw loop below
            const size_t row = (size_t)p * a.n_rows + r0 + r;
            int best = 0;
            float bestv = -1.f, pbest = 0.f;
            for (int j = 0; j < nout; ++j) {
                const float pj = cq.prob(outb[r * op + j]);
                cq.psum += pj;
                // q ~ Exp(1): injected, or -log(u) from the launch's Philox stream
                const float qj = a.device_eps ? -logf(u01(philox4x32_10(a.rng_counter, 0x9100u, (unsigned)((r0 + r) * nout + j), key).x))
                                              : a.eps[row * nout + j];
                const float v = pj / qj;
                if (v > bestv) { bestv = v; best = j; pbest = pj; }
            }
            a.out[row] = (float)best;
            if (a.env_out) a.env_out[row] = (float)best;
            if (a.out_logp) {
                const float qc = cq.clamped(pbest);
                // (REINFORCE records this value as the step's log-prob: the correctly rounded logarithm, so that a clamped row reads
                // log(eps) / log(1 - eps) to the bit as it does in the reference; logf is one ulp off at eps)
                a.out_logp[row] = D.cat_logits ? cq.logit(outb[r * op + best])                   // Categorical(logits=)
                                               : (D.algo == ALGO_REINFORCE ? (float)log((double)qc) : logf(qc));
            }
        }
        return;
    }
    for (int e = threadIdx.x; e < nv * nout; e += kWG) {
        const int r = e / nout, c = e - r * nout;
        const size_t o = ((size_t)p * a.n_rows + r0 + r) * nout + c;
        float v = outb[r * op + c];
        if (a.mode == ACTM_SAC_SAMPLE || a.mode == ACTM_PPO_SAMPLE) {
            const float ls = clamp_log_std(theta[N.extra_off + c]);
            const float sd = expf(ls);
            const float eps = a.eps ? a.eps[o] : (a.device_eps ? normal_at(0x9200u, (unsigned)((r0 + r) * nout + c)) : 0.f);
            const float u = v + sd * eps;
            if (a.mode == ACTM_SAC_SAMPLE) {
                v = tanhf(u);
            } else {
                const float du = u - v;
                if (a.out_logp) a.out_logp[o] = normal_logp(du, sd, ls);
                v = u;
            }
        }
        a.out[o] = v;
        if (a.env_out) {
            // action_ = clip(action * max_action [+ exploration noise], -max_action, max_action): TD3.py:412 (Gaussian),
            // SAC.py:528-533 (OU / Gaussian / none), PPO_with_tricks.py:529-530 (none)
            const float ma = a.max_action, sc = a.scale ? a.scale[p] : a.scale0;
            float x = v * ma;
            if (a.explore == EXPL_GAUSS) {
                x += sc * (normal_at(0x9300u, (unsigned)((r0 + r) * nout + c)) * (a.sigma * ma));
            } else if (a.explore == EXPL_OU) {
                float st = a.ou_state[o];
                if (a.flags && (a.flags[(size_t)p * a.n_rows + r0 + r] & 2)) st = 0.f;             // OUNoise.reset() at the episode's end
                st = st + (a.ou_theta * (0.f - st) + sqrtf(a.ou_dt) * a.ou_sigma * normal_at(0x9300u, (unsigned)((r0 + r) * nout + c)));
                a.ou_state[o] = st;
                x += (st * sc) * ma;
            }
            a.env_out[o] = fminf(fmaxf(x, -ma), ma);
        }
    }
}

// The same for the engines of the register-chained kernels (NetDesc::frag: parameters in fragment-image order): the net's
// images staged linearly into LDS, 64 rows per workgroup carried through the MLP in registers (device/chain_net.hpp), the
// head tile written to LDS for the shared epilogue.  Shape: 3 layers, hidden 128, <= 16 inputs and outputs, ReLU (what
// chained_shape() admits); grid = (ceil(n_rows / 64), learners).
// (the body as a device function: kernels_solo.hip runs it at the tail of its launches for the rollout loop's next select_action)
__device__ __forceinline__ void act_frag_body(const EngineDesc& D, const ActArgs& a, float* smem, int p, int r0) {
    const NetDesc& N = D.net[a.net];
    ChainNet C;
    C.init(smem);
    const int nv = min(64, a.n_rows - r0);
    const size_t off = (size_t)p * D.learner_stride + D.net_off[a.net];
    g_cf theta = as_global((a.use_target ? D.target : D.theta) + off);
    const int l0 = a.head * 3, K = a.in_dim;
    const int row = 16 * C.w + C.i16;
    f32x4 xb[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if (row < nv) {
        g_cf in = as_global(a.in + ((size_t)p * a.n_rows + r0 + row) * K);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * C.q + e < K) xb[0][e] = in[4 * C.q + e];
    }
    C.stage(theta, a.head, N.heads == 1 ? N.extra_n : 0);
    f32x4 z[1], h1[1][kHT], h2[1][kHT];
    C.forward<1>(xb, h1, h2, z);
    const bool th = (a.mode == ACTM_TANH || a.mode == ACTM_PPO_SAMPLE);
    lds_f outb = C.S.ea;                                               // [64][20]
    constexpr int op = 20;
#pragma unroll
    for (int r = 0; r < 4; ++r) outb[row * op + 4 * C.q + r] = th ? tanhf(z[0][r]) : z[0][r];
    __syncthreads();
    act_epilogue(D, a, N, theta, outb, op, nv, r0, p, N.L[l0 + 2].n);
}


}  // namespace frl
