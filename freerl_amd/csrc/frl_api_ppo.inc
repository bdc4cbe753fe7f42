// PPO entry points (included at the end of frl_api.hip).

#include "onpolicy_plan.hpp"

// The call's permutations into d_perm on the engine's stream: the caller's (`host`, narrowed by narrow_perms), ppo_perm_kernel's, or past
// 8192 rows the host shuffle's.  One rng_counter value per drawn call.  `host` is pageable: it must outlive the copy (the callers synchronise)
static int onpolicy_perms(frl_engine* e, const OnpolicyCall& c, std::vector<int>* host) {
    if (c.perms == PERM_DEVICE) {
        hipLaunchKernelGGL(ppo_perm_kernel, dim3(c.K, (unsigned)c.units), dim3(256), (size_t)c.Tpad * sizeof(unsigned long long), e->stream,
                           e->d_perm, c.T, c.Tpad, (unsigned long long)(++e->rng_counter), (unsigned long long)e->h.seed);
        return FRL_OK;
    }
    if (c.perms == PERM_HOST) host_shuffle(e->h.seed, ++e->rng_counter, c.units * c.K, c.T, host);
    HIP_TRY(hipMemcpyAsync(e->d_perm, host->data(), host->size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    return FRL_OK;
}

// flush_stage (which takes no rng_counter value), then d_ppo and d_perm grown to the layout's totals
static int onpolicy_scratch(frl_engine* e, size_t floats, size_t ints) {
    const int rc = flush_stage(e);
    if (rc) return rc;
    HIP_TRY(e->mem.grow(&e->d_ppo, e->ppo_cap, floats, MEM_DEVICE));
    HIP_TRY(e->mem.grow(&e->d_perm, e->perm_cap, ints, MEM_DEVICE));
    return FRL_OK;
}

extern "C" int frl_ppo_learn(frl_engine* e, const frl_ppo_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_PPO) return wrong_engine(h, "frl_ppo_learn");
    // everything that can refuse the call comes before anything is flushed, grown, uploaded or launched
    OnpolicyCall c;
    std::string why;
    std::vector<int> perm;      // permutations: the caller's np.random.permutation draws (PPO_with_tricks.py:320), else drawn (onpolicy_perms)
    if (const int rc = plan_onpolicy(ONP_PPO, h.capacity, h.batch_max, h.P, args->horizon, args->minibatch, args->k_epochs, args->perms != nullptr, &c, &why))
        return fail(rc, "%s", why.c_str());
    if (args->gae_mode != 0 && args->gae_mode != 1) return fail(FRL_ERR_INVALID, "gae_mode %d (0 or 1)", args->gae_mode);
    if (args->gae_mode == 1) {
        if (!args->last_value) return fail(FRL_ERR_INVALID, "gae_mode 1 needs last_value");
        if (h.rec.extra < 3) return fail(FRL_ERR_STATE, "gae_mode 1 needs the value column: extra_cols = log-probs + value + adv_done");
    }
    if (args->perms && narrow_perms(args->perms, c.perm_n(), c.T, &perm, &why)) return fail(FRL_ERR_INVALID, "%s", why.c_str());
    const int T = c.T;
    const size_t P = h.P;
    const PpoLayout L = ppo_layout(c);
    if (const int rc = onpolicy_scratch(e, L.floats, L.ints)) return rc;
    if (const int rc = onpolicy_perms(e, c, &perm)) return rc;
    PpoArgs a;
    memset(&a, 0, sizeof a);
    a.horizon = T; a.minibatch = c.mb; a.k_epochs = c.K; a.adv_norm = args->adv_norm;
    a.gamma = args->gamma; a.lmbda = args->lmbda; a.clip = args->clip; a.ent_coef = args->ent_coef;
    a.actor_lr = args->actor_lr; a.critic_lr = args->critic_lr;
    a.adam_eps = args->adam_eps > 0 ? args->adam_eps : 1e-8f;
    a.beta1 = 0.9f; a.beta2 = 0.999f;
    a.clip_norm = args->clip_norm;
    a.optimizer = args->optimizer;
    a.td = e->d_ppo + L.td; a.vs = e->d_ppo + L.vs; a.adv_raw = e->d_ppo + L.adv_raw; a.adv = e->d_ppo + L.adv;
    a.vtarget = e->d_ppo + L.vtarget; a.trace = e->d_ppo + L.trace;
    a.perm = e->d_perm;
    if (h.obs_norm_on)      // learn(): obs = norm(obs) over the whole horizon updates the statistics (PPO_with_tricks.py:297-299)
        hipLaunchKernelGGL(obsnorm_kernel, dim3(h.P), dim3(256), 0, e->stream, e->d, T, 1, 0);
    if (args->gae_mode == 1) {
        a.gamma_d = args->gae_gamma != 0.0 ? args->gae_gamma : (double)args->gamma;
        a.lmbda_d = args->gae_lmbda != 0.0 ? args->gae_lmbda : (double)args->lmbda;
        HIP_TRY(hipMemcpyAsync(a.td, args->last_value, P * sizeof(float), hipMemcpyHostToDevice, e->stream));   // td is free in this mode
        a.last_value = a.td;
        hipLaunchKernelGGL(ppo_gae_sb3_kernel, dim3(h.P), dim3(256), 0, e->stream, e->d, a);
    } else {
        hipLaunchKernelGGL(ppo_values_kernel, dim3((T + h.rc - 1) / h.rc, h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
        hipLaunchKernelGGL(ppo_gae_kernel, dim3(h.P), dim3(256), 0, e->stream, e->d, a);
    }
    // the on-chip kernel (kernels_ppo2.hip) covers the reference's standard shape; everything else runs the streaming one
    const NetDesc &NA = h.net[0], &NC = h.net[1];
    const bool v2 = h.hidden == 128 && NA.n_layers == 3 && NC.n_layers == 3 && NA.L[0].k_pad <= 32 && NA.L[2].n_pad == 16 &&
                    NC.L[2].n_pad == 16 && !h.beta_actor && args->optimizer == 0 && NA.hidden_act == NC.hidden_act &&
                    (NA.hidden_act == ACT_RELU || NA.hidden_act == ACT_TANH) && !env_set("FRL_PPO_STREAMING");
    if (v2) {
        const int k0b = NA.L[0].k_pad / 16;
        const size_t lb = (size_t)ppo2_lds_floats(k0b) * sizeof(float);
        const bool th = NA.hidden_act == ACT_TANH;
        if (k0b == 1 && !th) hipLaunchKernelGGL(ppo_update_v2_k1_relu, dim3(h.P, 2), dim3(256), lb, e->stream, e->d, a);
        else if (k0b == 2 && !th) hipLaunchKernelGGL(ppo_update_v2_k2_relu, dim3(h.P, 2), dim3(256), lb, e->stream, e->d, a);
        else if (k0b == 1) hipLaunchKernelGGL(ppo_update_v2_k1_tanh, dim3(h.P, 2), dim3(256), lb, e->stream, e->d, a);
        else hipLaunchKernelGGL(ppo_update_v2_k2_tanh, dim3(h.P, 2), dim3(256), lb, e->stream, e->d, a);
    } else {
        hipLaunchKernelGGL(ppo_update_kernel, dim3(h.P, 2), dim3(256), e->lds_bytes, e->stream, e->d, a);
    }
    HIP_TRY(hipGetLastError());
    ++e->param_version;      // as its siblings do; read only on wide and solow engines, which a PPO engine never is: nothing observable changes
    HIP_TRY(hipStreamSynchronize(e->stream));      // `perm` (pageable) must outlive the copy
    if (args->adv_out) HIP_TRY(hipMemcpy(args->adv_out, a.adv_raw, c.rows() * sizeof(float), hipMemcpyDeviceToHost));
    if (args->vtarget_out) HIP_TRY(hipMemcpy(args->vtarget_out, a.vtarget, c.rows() * sizeof(float), hipMemcpyDeviceToHost));
    if (args->loss_trace_out) HIP_TRY(hipMemcpy(args->loss_trace_out, a.trace, c.trace_n() * sizeof(float), hipMemcpyDeviceToHost));
    // Buffer_for_PPO.clear() (PPO_with_tricks.py:354): counters only
    for (int p = 0; p < h.P; ++p) { e->index[p] = 0; e->size[p] = 0; }
    return FRL_OK;
}

// Algorithmic work of one frl_ppo_learn for ALL learners (DESIGN.md "Roofline"): flops = 2 * rows * sum(in*out) per forward
// pass and twice that per backward pass (dW of every layer + dX of all but the first are counted as 2x like SURVEY §8d);
// rows = 2 * horizon through the critic for V(s), V(s') plus K_epochs * horizon through actor and critic forward +
// backward.  bytes = the rows gathered per pass + theta, m, v of both nets read and written ONCE per learn() (they stay on
// chip in between) + the GAE streams.
extern "C" int frl_ppo_work(const frl_engine* e, int horizon, int k_epochs, double* flops_out, double* bytes_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_PPO) return wrong_engine(h, "frl_ppo_work");
    auto macs = [](const NetDesc& N) { double s = 0; for (int i = 0; i < N.n_layers; ++i) s += (double)N.L[i].n * N.L[i].k; return s; };
    const double T = horizon, K = k_epochs, ma = macs(h.net[0]), mc = macs(h.net[1]);
    const RecordDesc& R = h.rec;
    const double fl = 2.0 * (2.0 * T) * mc + 2.0 * (K * T) * (ma + mc) * 3.0;
    const double row_bytes = 4.0 * (R.obs_total + R.act_total + R.extra + 2);
    const double by = 4.0 * T * (2.0 * R.obs_total + 2) + K * T * row_bytes + 24.0 * (h.net[0].n_params + h.net[1].n_params) + 5.0 * 4.0 * T;
    if (flops_out) *flops_out = fl * h.P;
    if (bytes_out) *bytes_out = by * h.P;
    return FRL_OK;
}

#ifdef FRL_PPO_TIMING
// developer build only (tools/ppo_timing.py): cycles per section of ppo_update_kernel, [actor | critic][8]
extern "C" int frl_debug_ppo_clocks(long long* out) {
    hipDeviceSynchronize();
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(frl::g_ppo_clk), sizeof(long long) * 16, 0, hipMemcpyDeviceToHost);
}
#endif

#ifdef FRL_PPO_TIMING_SPLIT
// developer build only, the quick form (tools/build_unit_timing.sh <unit>: ONE kernels_*.hip compiled with -DFRL_PPO_TIMING
// -DFRL_CLK_COPY=1, this unit with -DFRL_PPO_TIMING_SPLIT, the other objects as built): the stamps live in that unit, which copies them out
namespace frl { __global__ void frl_clk_copy_kernel(long long* out); }
extern "C" int frl_debug_ppo_clocks(long long* out) {
    long long* d = nullptr;
    if (hipMalloc((void**)&d, 16 * sizeof(long long)) != hipSuccess) return -1;
    hipDeviceSynchronize();
    hipLaunchKernelGGL(frl::frl_clk_copy_kernel, dim3(1), dim3(64), 0, 0, d);
    const int rc = (int)hipMemcpy(out, d, 16 * sizeof(long long), hipMemcpyDeviceToHost);
    hipFree(d);
    return rc;
}
#endif

#ifdef FRL_WIDE_TIMING
// developer build only (tools/wide_timing.py): cycles per section of kernels_criticw.hip / kernels_actorw.hip, [critic | actor][16]
extern "C" int frl_debug_wide_clocks(long long* out) {
    hipDeviceSynchronize();
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(frl::g_wide_clk), sizeof(long long) * 32, 0, hipMemcpyDeviceToHost);
}
#endif

extern "C" int frl_gae(frl_engine* e, const float* td_delta_dev, const float* adv_done_dev, int n_seq, int horizon,
                       float gamma, float lmbda, float* adv_out_dev) {
    ENG(e);
    if (!td_delta_dev || !adv_done_dev || !adv_out_dev || n_seq < 1 || horizon < 1) return fail(FRL_ERR_INVALID, "bad argument");
    hipLaunchKernelGGL(gae_dense_kernel, dim3(n_seq), dim3(256), 0, e->stream, td_delta_dev, adv_done_dev, horizon,
                       gamma * lmbda, adv_out_dev);
    HIP_TRY(hipGetLastError());
    return FRL_OK;
}
