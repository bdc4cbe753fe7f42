// PPO entry points (included at the end of frl_api.hip).

static int ppo_scratch(frl_engine* e, int T, int k_epochs, int n_mb) {
    const size_t P = e->h.P;
    HIP_TRY(e->mem.grow(&e->d_ppo, e->ppo_cap, P * ((size_t)5 * T + (size_t)k_epochs * n_mb * 2), MEM_DEVICE));
    HIP_TRY(e->mem.grow(&e->d_perm, e->perm_cap, P * (size_t)k_epochs * T, MEM_DEVICE));
    return FRL_OK;
}

static inline unsigned long long splitmix64(unsigned long long& s) {
    unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

extern "C" int frl_ppo_learn(frl_engine* e, const frl_ppo_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_PPO) return wrong_engine(h, "frl_ppo_learn");
    const int T = args->horizon, mb = args->minibatch, K = args->k_epochs;
    if (T < 2 || T > h.capacity) return fail(FRL_ERR_INVALID, "horizon %d outside [2, capacity %d]", T, h.capacity);
    if (mb < 1 || mb > h.batch_max) return fail(FRL_ERR_INVALID, "minibatch %d outside [1,%d]", mb, h.batch_max);
    if (K < 1) return fail(FRL_ERR_INVALID, "k_epochs must be >= 1");
    if (args->gae_mode != 0 && args->gae_mode != 1) return fail(FRL_ERR_INVALID, "gae_mode %d (0 or 1)", args->gae_mode);
    if (args->gae_mode == 1) {
        if (!args->last_value) return fail(FRL_ERR_INVALID, "gae_mode 1 needs last_value");
        if (h.rec.extra < 3) return fail(FRL_ERR_STATE, "gae_mode 1 needs the value column: extra_cols = log-probs + value + adv_done");
    }
    const int n_mb = (T + mb - 1) / mb;
    int rc = flush_stage(e);
    if (rc) return rc;
    rc = ppo_scratch(e, T, K, n_mb);
    if (rc) return rc;
    const size_t P = h.P;
    // permutations: caller's np.random.permutation draws (PPO_with_tricks.py:320), else drawn on the device (a sort of random
    // keys per learner and epoch; horizons beyond 8192 rows: a host Fisher-Yates)
    int Tpad = 2;
    while (Tpad < T) Tpad <<= 1;
    const bool dev_perm = !args->perms && Tpad <= 8192;
    std::vector<int> perm(dev_perm ? 0 : P * (size_t)K * T);
    if (dev_perm) {
        hipLaunchKernelGGL(ppo_perm_kernel, dim3(K, h.P), dim3(256), (size_t)Tpad * sizeof(unsigned long long), e->stream,
                           e->d_perm, T, Tpad, (unsigned long long)(++e->rng_counter), (unsigned long long)h.seed);
    } else if (args->perms) {
        for (size_t i = 0; i < perm.size(); ++i) {
            const int64_t v = args->perms[i];
            if (v < 0 || v >= T) return fail(FRL_ERR_INVALID, "permutation entry %lld outside [0,%d)", (long long)v, T);
            perm[i] = (int)v;
        }
    } else {
        unsigned long long s = h.seed ^ (0xD1B54A32D192ED03ull * (++e->rng_counter));
        for (size_t blk = 0; blk < P * (size_t)K; ++blk) {
            int* q = perm.data() + blk * T;
            for (int i = 0; i < T; ++i) q[i] = i;
            for (int i = T - 1; i > 0; --i) {
                const int j = (int)(splitmix64(s) % (unsigned long long)(i + 1));
                std::swap(q[i], q[j]);
            }
        }
    }
    if (!dev_perm) HIP_TRY(hipMemcpyAsync(e->d_perm, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    PpoArgs a;
    memset(&a, 0, sizeof a);
    a.horizon = T; a.minibatch = mb; a.k_epochs = K; a.adv_norm = args->adv_norm;
    a.gamma = args->gamma; a.lmbda = args->lmbda; a.clip = args->clip; a.ent_coef = args->ent_coef;
    a.actor_lr = args->actor_lr; a.critic_lr = args->critic_lr;
    a.adam_eps = args->adam_eps > 0 ? args->adam_eps : 1e-8f;
    a.beta1 = 0.9f; a.beta2 = 0.999f;
    a.clip_norm = args->clip_norm;
    a.optimizer = args->optimizer;
    float* q = e->d_ppo;
    a.td = q; q += P * T;
    a.vs = q; q += P * T;
    a.adv_raw = q; q += P * T;
    a.adv = q; q += P * T;
    a.vtarget = q; q += P * T;
    a.trace = q;
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
    HIP_TRY(hipStreamSynchronize(e->stream));      // `perm` (pageable) must outlive the copy
    if (args->adv_out) HIP_TRY(hipMemcpy(args->adv_out, a.adv_raw, P * T * sizeof(float), hipMemcpyDeviceToHost));
    if (args->vtarget_out) HIP_TRY(hipMemcpy(args->vtarget_out, a.vtarget, P * T * sizeof(float), hipMemcpyDeviceToHost));
    if (args->loss_trace_out) HIP_TRY(hipMemcpy(args->loss_trace_out, a.trace, P * (size_t)K * n_mb * 2 * sizeof(float), hipMemcpyDeviceToHost));
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
