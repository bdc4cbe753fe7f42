// GAIL's policy side (GAIL_file/PPO2.py) on an ALGO_GAIL_PPO engine (included at the end of frl_api.hip; kernels_gail_ppo.hip).

extern "C" int frl_log_std_range_set(frl_engine* e, float lo, float hi) {
    ENG(e);
    if (e->h.algo != ALGO_GAIL_PPO) return wrong_engine(e->h, "frl_log_std_range_set");
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return fail(FRL_ERR_INVALID, "log_std range [%g, %g]: finite bounds with lo < hi", (double)lo, (double)hi);
    e->h.log_std_min = lo;
    e->h.log_std_max = hi;
    return push_desc(e);
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
    OnpolicyCall c;
    std::string why;
    std::vector<int> perm;      // permutations: the caller's torch.randperm draws (PPO2.py:266), else drawn as frl_ppo_learn draws them (onpolicy_perms)
    if (const int rc = plan_onpolicy(ONP_GAIL_PPO, h.capacity, h.batch_max, h.P, args->horizon, args->minibatch, args->k_epochs, args->perms != nullptr, &c, &why))
        return fail(rc, "%s", why.c_str());
    if (args->perms && narrow_perms(args->perms, c.perm_n(), c.T, &perm, &why)) return fail(FRL_ERR_INVALID, "%s", why.c_str());
    const int T = c.T;
    const size_t P = h.P, PT = c.rows();
    // scratch: vs, logp_old, td, adv_raw, adv, returns, rewards [P][T] each, last_value [P], the loss trace
    const GailPpoLayout L = gail_ppo_layout(c);
    if (const int rc = onpolicy_scratch(e, L.floats, L.ints)) return rc;
    GailPpoArgs a;
    memset(&a, 0, sizeof a);
    a.horizon = T; a.minibatch = c.mb; a.k_epochs = c.K;
    a.gamma = args->gamma;
    a.c = (float)((double)args->gamma * (double)args->lam);      // `gamma * lam` is a product of Python floats before it meets a tensor (:213)
    a.clip = args->clip; a.ent_weight = args->ent_weight; a.value_loss_coef = args->value_loss_coef;
    a.p_lr = args->p_lr; a.v_lr = args->v_lr; a.clip_norm = args->clip_norm;
    a.vs = e->d_ppo + L.vs; a.logp_old = e->d_ppo + L.logp_old; a.td = e->d_ppo + L.td; a.adv_raw = e->d_ppo + L.adv_raw; a.adv = e->d_ppo + L.adv;
    a.returns = e->d_ppo + L.returns; a.trace = e->d_ppo + L.trace;
    float *d_rew = e->d_ppo + L.rewards, *d_last = e->d_ppo + L.last_value;
    a.perm = e->d_perm;
    a.last_value = d_last;
    if (args->last_value) HIP_TRY(hipMemcpyAsync(d_last, args->last_value, P * sizeof(float), hipMemcpyHostToDevice, e->stream));
    else HIP_TRY(hipMemsetAsync(d_last, 0, P * sizeof(float), e->stream));
    if (args->rewards) {      // the discriminator's rewards in place of the ring's column: one upload of 4 T bytes per learner
        HIP_TRY(hipMemcpyAsync(d_rew, args->rewards, PT * sizeof(float), hipMemcpyHostToDevice, e->stream));
        a.rewards = d_rew;
    }
    if (const int rc = onpolicy_perms(e, c, &perm)) return rc;
    hipLaunchKernelGGL(gail_ppo_prepare_kernel, dim3((T + h.rc - 1) / h.rc, h.P), dim3(256), e->lds_bytes, e->stream, e->d, a);
    hipLaunchKernelGGL(gail_ppo_gae_kernel, dim3(h.P), dim3(256), 0, e->stream, e->d, a);
    hipLaunchKernelGGL(gail_ppo_update_kernel, dim3(h.P, 2), dim3(256), e->lds_bytes, e->stream, e->d, a);
    HIP_TRY(hipGetLastError());
    ++e->param_version;
    HIP_TRY(hipStreamSynchronize(e->stream));      // the pageable uploads (`perm`, the caller's arrays) must outlive their copies
    if (args->adv_out) HIP_TRY(hipMemcpy(args->adv_out, a.adv_raw, PT * sizeof(float), hipMemcpyDeviceToHost));
    if (args->returns_out) HIP_TRY(hipMemcpy(args->returns_out, a.returns, PT * sizeof(float), hipMemcpyDeviceToHost));
    if (args->logp_old_out) HIP_TRY(hipMemcpy(args->logp_old_out, a.logp_old, PT * sizeof(float), hipMemcpyDeviceToHost));
    if (args->loss_trace_out) HIP_TRY(hipMemcpy(args->loss_trace_out, a.trace, c.trace_n() * sizeof(float), hipMemcpyDeviceToHost));
    // (the ring's cursors stay: the reference clears `memory` in its loop, not in PPO_learn — PPO2.py:458)
    return FRL_OK;
}
