// GAIL's policy side (GAIL_file/PPO2.py) on an ALGO_GAIL_PPO engine (included at the end of frl_api.hip; kernels_gail_ppo.hip).

extern "C" int frl_log_std_range_set(frl_engine* e, float lo, float hi) {
    ENG(e);
    if (e->h.algo != ALGO_GAIL_PPO) return wrong_engine(e->h, "frl_log_std_range_set");
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return fail(FRL_ERR_INVALID, "log_std range [%g, %g]: finite bounds with lo < hi", (double)lo, (double)hi);
    e->h.log_std_min = lo;
    e->h.log_std_max = hi;
    HIP_TRY(hipStreamSynchronize(e->stream));      // (no launch may be reading the descriptor while it changes)
    HIP_TRY(hipMemcpy(e->d, &e->h, sizeof e->h, hipMemcpyHostToDevice));
    return FRL_OK;
}

extern "C" int frl_log_std_range_get(const frl_engine* e, float* lo_out, float* hi_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    if (e->h.algo != ALGO_GAIL_PPO) return wrong_engine(e->h, "frl_log_std_range_get");
    if (lo_out) *lo_out = e->h.log_std_min;
    if (hi_out) *hi_out = e->h.log_std_max;
    return FRL_OK;
}

extern "C" int frl_gail_ppo_learn(frl_engine* e, const frl_gail_ppo_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_GAIL_PPO) return wrong_engine(h, "frl_gail_ppo_learn");
    const int T = args->horizon, mb = args->minibatch, K = args->k_epochs;
    if (T < 2) return fail(FRL_ERR_INVALID, "horizon %d < 2: the unbiased std of one advantage is NaN", T);
    if (T > h.capacity) return fail(FRL_ERR_INVALID, "horizon %d > capacity %d", T, h.capacity);
    if (mb < 1 || mb > h.batch_max) return fail(FRL_ERR_INVALID, "minibatch %d outside [1,%d]", mb, h.batch_max);
    if (K < 1) return fail(FRL_ERR_INVALID, "k_epochs must be >= 1");
    const size_t P = h.P;
    const int n_mb = (T + mb - 1) / mb;
    // permutations: the caller's torch.randperm draws (PPO2.py:266), else drawn as frl_ppo_learn draws them (ppo_perm_kernel; horizons
    // beyond 8192 rows: a host Fisher-Yates).  Checked before anything is launched or uploaded
    int Tpad = 2;
    while (Tpad < T) Tpad <<= 1;
    const bool dev_perm = !args->perms && Tpad <= 8192;
    std::vector<int> perm(dev_perm ? 0 : P * (size_t)K * T);
    if (args->perms) {
        for (size_t i = 0; i < perm.size(); ++i) {
            const int64_t v = args->perms[i];
            if (v < 0 || v >= T) return fail(FRL_ERR_INVALID, "permutation entry %lld outside [0,%d)", (long long)v, T);
            perm[i] = (int)v;
        }
    } else if (!dev_perm) {
        unsigned long long s = h.seed ^ (0xD1B54A32D192ED03ull * (++e->rng_counter));
        for (size_t blk = 0; blk < P * (size_t)K; ++blk) {
            int* q = perm.data() + blk * T;
            for (int i = 0; i < T; ++i) q[i] = i;
            for (int i = T - 1; i > 0; --i) std::swap(q[i], q[(int)(splitmix64(s) % (unsigned long long)(i + 1))]);
        }
    }
    int rc = flush_stage(e);
    if (rc) return rc;
    // scratch: vs, logp_old, td, adv_raw, adv, returns, rewards [P][T] each, last_value [P], the loss trace
    const size_t PT = P * (size_t)T;
    HIP_TRY(e->mem.grow(&e->d_ppo, e->ppo_cap, 7 * PT + P + P * (size_t)K * n_mb * 2, MEM_DEVICE));
    HIP_TRY(e->mem.grow(&e->d_perm, e->perm_cap, P * (size_t)K * T, MEM_DEVICE));
    GailPpoArgs a;
    memset(&a, 0, sizeof a);
    a.horizon = T; a.minibatch = mb; a.k_epochs = K;
    a.gamma = args->gamma;
    a.c = (float)((double)args->gamma * (double)args->lam);      // `gamma * lam` is a product of Python floats before it meets a tensor (:213)
    a.clip = args->clip; a.ent_weight = args->ent_weight; a.value_loss_coef = args->value_loss_coef;
    a.p_lr = args->p_lr; a.v_lr = args->v_lr; a.clip_norm = args->clip_norm;
    float* q = e->d_ppo;
    a.vs = q; q += PT;
    a.logp_old = q; q += PT;
    a.td = q; q += PT;
    a.adv_raw = q; q += PT;
    a.adv = q; q += PT;
    a.returns = q; q += PT;
    float* d_rew = q; q += PT;
    float* d_last = q; q += P;
    a.trace = q;
    a.perm = e->d_perm;
    a.last_value = d_last;
    if (args->last_value) HIP_TRY(hipMemcpyAsync(d_last, args->last_value, P * sizeof(float), hipMemcpyHostToDevice, e->stream));
    else HIP_TRY(hipMemsetAsync(d_last, 0, P * sizeof(float), e->stream));
    if (args->rewards) {      // the discriminator's rewards in place of the ring's column: one upload of 4 T bytes per learner
        HIP_TRY(hipMemcpyAsync(d_rew, args->rewards, PT * sizeof(float), hipMemcpyHostToDevice, e->stream));
        a.rewards = d_rew;
    }
    if (dev_perm)
        hipLaunchKernelGGL(ppo_perm_kernel, dim3(K, h.P), dim3(256), (size_t)Tpad * sizeof(unsigned long long), e->stream, e->d_perm, T, Tpad,
                           (unsigned long long)(++e->rng_counter), (unsigned long long)h.seed);
    else
        HIP_TRY(hipMemcpyAsync(e->d_perm, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(gail_ppo_prepare_kernel, dim3((T + h.rc - 1) / h.rc, h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
    hipLaunchKernelGGL(gail_ppo_gae_kernel, dim3(h.P), dim3(256), 0, e->stream, e->d, a);
    hipLaunchKernelGGL(gail_ppo_update_kernel, dim3(h.P, 2), dim3(256), e->lds_bytes, e->stream, e->d, a);
    HIP_TRY(hipGetLastError());
    ++e->param_version;
    HIP_TRY(hipStreamSynchronize(e->stream));      // the pageable uploads (`perm`, the caller's arrays) must outlive their copies
    if (args->adv_out) HIP_TRY(hipMemcpy(args->adv_out, a.adv_raw, PT * sizeof(float), hipMemcpyDeviceToHost));
    if (args->returns_out) HIP_TRY(hipMemcpy(args->returns_out, a.returns, PT * sizeof(float), hipMemcpyDeviceToHost));
    if (args->logp_old_out) HIP_TRY(hipMemcpy(args->logp_old_out, a.logp_old, PT * sizeof(float), hipMemcpyDeviceToHost));
    if (args->loss_trace_out) HIP_TRY(hipMemcpy(args->loss_trace_out, a.trace, P * (size_t)K * n_mb * 2 * sizeof(float), hipMemcpyDeviceToHost));
    // (the ring's cursors stay: the reference clears `memory` in its loop, not in PPO_learn — PPO2.py:458)
    return FRL_OK;
}
