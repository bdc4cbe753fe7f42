// frl_gail_learn / frl_gail_reward (include/freerl_hip.h): GAIL.trian_D and GAIL.compute_reward (GAIL_file/GAIL.py:62-120) for a
// population.  Included by frl_api.hip.
//
// Launch chain of frl_gail_learn: [gail_draw_kernel: n_expert ring rows per learner WITH replacement when idx is NULL] ->
// gail_disc_kernel (row chunks over the n_expert + n_policy rows) -> reduce + Adam (launch_adam: net 0, statistics in the actor slots,
// the call's betas, no clipping, no soft update: there is no target) -> gail_stats_kernel (the six results per learner).

extern "C" int frl_gail_learn(frl_engine* e, const frl_gail_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_GAIL) return wrong_engine(h, "frl_gail_learn");
    const int E = args->n_expert, NP = args->n_policy, P = h.P;
    const int IN = h.rec.obs_dim[0] + h.rec.act_dim[0];
    if (E < 1 || E > h.batch_max) return fail(FRL_ERR_INVALID, "n_expert %d outside [1, batch_max %d]", E, h.batch_max);
    if (NP < 1 || NP > h.batch_max) return fail(FRL_ERR_INVALID, "n_policy %d outside [1, batch_max %d]", NP, h.batch_max);
    if (args->gp != 0 && args->gp != 1) return fail(FRL_ERR_INVALID, "gp %d must be 0 or 1", args->gp);
    for (const float v : {args->gp_weight, args->lr, args->beta1, args->beta2, args->adam_eps})
        if (!(v == v)) return fail(FRL_ERR_INVALID, "gp_weight / lr / beta1 / beta2 / adam_eps is NaN");
    if (args->gp_weight < 0.f) return fail(FRL_ERR_INVALID, "gp_weight %g must be >= 0", (double)args->gp_weight);
    if (args->beta1 < 0.f || args->beta1 >= 1.f || args->beta2 < 0.f || args->beta2 >= 1.f)
        return fail(FRL_ERR_INVALID, "betas (%g, %g) outside [0, 1)", (double)args->beta1, (double)args->beta2);
    if (!args->policy_rows) return fail(FRL_ERR_INVALID, "policy_rows is NULL");
    int min_size = h.capacity;
    for (int p = 0; p < P; ++p) min_size = std::min(min_size, e->size[p]);
    if (min_size < 1) return fail(FRL_ERR_STATE, "a learner's ring is empty: store the expert rows first");
    if (args->idx)
        for (int p = 0; p < P; ++p)
            for (int i = 0; i < E; ++i) {
                const int64_t v = args->idx[(size_t)p * E + i];
                if (v < 0 || v >= e->size[p]) return fail(FRL_ERR_STATE, "idx entry %lld of learner %d is not one of its %d stored rows", (long long)v, p, e->size[p]);
            }
    int rc = flush_stage(e);
    if (rc) return rc;
    rc = upload_idx_noise(e, args->idx, nullptr, E, 1);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));                           // pinned staging reuse
    const size_t pitch = (size_t)h.batch_max * IN, rn = (size_t)NP * IN;
    for (int p = 0; p < P; ++p) {
        memcpy(e->h_gail_rows + p * pitch, args->policy_rows + p * rn, rn * sizeof(float));
        HIP_TRY(hipMemcpyAsync(h.gail_rows + p * pitch, e->h_gail_rows + p * pitch, rn * sizeof(float), hipMemcpyHostToDevice, e->stream));
    }
    GailArgs a;
    memset(&a, 0, sizeof a);
    a.n_expert = E; a.n_policy = NP; a.gp = args->gp; a.gp_weight = args->gp_weight;
    a.size = min_size; a.p0 = 0; a.p_count = P;
    ++e->param_version;
    const int ns = rowchunk_ns(h, E + NP);
    if (!args->idx) {
        a.rng_counter = e->rng_counter++;
        prof_begin(e, PK_DRAW);
        hipLaunchKernelGGL(gail_draw_kernel, dim3(P), dim3(256), 0, e->stream, e->d, a);
        prof_end(e);
    }
    AdamArgs ad{};
    ad.which = 1;                                  // net 0, statistics in the actor slots (gail_stats_kernel rewrites the loss slot)
    ad.batch = E + NP;
    ad.lr = args->lr; ad.eps = args->adam_eps; ad.beta1 = args->beta1; ad.beta2 = args->beta2;
    ad.clip = 0.f; ad.soft = 0;
    launch_rowchunk_update(e, e->stream, P, 0, ns, ad, gail_disc_kernel, a);
    hipLaunchKernelGGL(gail_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, e->stream, e->d, a, ns);
    HIP_TRY(hipGetLastError());
    if (!args->out && !args->idx_out) return FRL_OK;
    std::vector<float> res((size_t)P * 8);
    std::vector<int> rows;
    if (args->out) HIP_TRY(hipMemcpyAsync(res.data(), h.gail_out, res.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (args->idx_out) {
        rows.resize((size_t)P * h.batch_max);
        HIP_TRY(hipMemcpyAsync(rows.data(), h.idx, rows.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int p = 0; p < P; ++p) {
        for (int i = 0; args->out && i < 6; ++i) args->out[(size_t)p * 6 + i] = res[(size_t)p * 8 + i];
        for (int i = 0; args->idx_out && i < E; ++i) args->idx_out[(size_t)p * E + i] = rows[(size_t)p * h.batch_max + i];
    }
    return FRL_OK;
}

extern "C" int frl_gail_reward(frl_engine* e, int gp, int n_rows, const float* rows_host, float* reward_out) {
    ENG(e);
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_GAIL) return wrong_engine(h, "frl_gail_reward");
    if (gp != 0 && gp != 1) return fail(FRL_ERR_INVALID, "gp %d must be 0 or 1", gp);
    if (n_rows < 1 || !rows_host || !reward_out) return fail(FRL_ERR_INVALID, "bad argument");
    const int IN = h.rec.obs_dim[0] + h.rec.act_dim[0];
    const size_t rows = (size_t)h.P * n_rows, in_n = rows * IN;
    int rc = act_scratch(e, in_n, rows);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_act_in, rows_host, in_n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(gail_forward_kernel, dim3((n_rows + h.rc - 1) / h.rc, h.P), dim3(256), e->lds_bytes, e->stream, e->d, gp ? 2 : 1, n_rows,
                       (const float*)e->d_act_in, e->d_act_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(reward_out, e->d_act_out, rows * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return FRL_OK;
}
