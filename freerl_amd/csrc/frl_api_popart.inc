// frl_popart_ddpg_learn, frl_popart_get and frl_popart_set (include/freerl_hip.h): DDPG.learn with trick['popart']
// (DDPG_file/DDPG_simple_with_tricks.py:244-292) for a population.  Included by frl_api.hip.
//
// Launch chain: [draw_kernel: `rows` distinct ring rows per learner when idx is NULL] -> popart_target_kernel (y with the old statistics,
// parked; sum y, sum y^2 per workgroup) -> popart_critic_kernel (the batch's statistics step derived by every workgroup, the normalised TD
// delta, the lower critic's gradient, the upper layer's two) -> popart_step_kernel (lower critic: reduce + clip 0.5 + Adam + soft update;
// then pop, the upper layer's clip and Adam, the statistics written back) -> popart_actor_kernel (through both just stepped) ->
// popart_step_kernel (actor, and the outputs).  The reference moves both targets after both steps (:281-292); the actor step reads
// neither target, so folding each soft update into its net's step ends where the reference does.

static int popart_engine(frl_engine* e, int learner, const char* who) {
    if (e->h.algo != ALGO_DDPG_POPART) return wrong_engine(e->h, who);
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner out of range");
    return FRL_OK;
}

extern "C" int frl_popart_get(frl_engine* e, int learner, float* out5) {
    ENG(e);
    if (!out5) return fail(FRL_ERR_INVALID, "out5 is NULL");
    if (const int rc = popart_engine(e, learner, "frl_popart_get")) return rc;
    HIP_TRY(hipMemcpyAsync(out5, e->h.popart + popart_offset(e->h, learner), 5 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return FRL_OK;
}

extern "C" int frl_popart_set(frl_engine* e, int learner, const float* in5) {
    ENG(e);
    if (!in5) return fail(FRL_ERR_INVALID, "in5 is NULL");
    if (const int rc = popart_engine(e, learner, "frl_popart_set")) return rc;
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(in5[i])) return fail(FRL_ERR_INVALID, "frl_popart_set: value %d of {W, b, sigma, mu, nu} is not finite", i);
    if (!(in5[POP_SIGMA] > 0.f)) return fail(FRL_ERR_INVALID, "frl_popart_set: sigma %g must be > 0", (double)in5[POP_SIGMA]);
    HIP_TRY(hipMemcpyAsync(e->h.popart + popart_offset(e->h, learner), in5, 5 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));      // (in5 is the caller's, pageable)
    ++e->param_version;
    return FRL_OK;
}

extern "C" int frl_popart_ddpg_learn(frl_engine* e, const frl_popart_ddpg_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_DDPG_POPART) return wrong_engine(h, "frl_popart_ddpg_learn");
    const int P = h.P;
    e->knobs = learn_knobs();
    PopartPlan pl;
    std::string why;
    if (const int prc = plan_popart_ddpg(h, e->size.data(), *args, &pl, &e->idx_narrow, &why)) return fail(prc, "%s", why.c_str());
    int rc = flush_stage(e);
    if (rc) return rc;
    if (args->idx) { rc = upload_idx(e, e->idx_narrow, 1, pl.rows); if (rc) return rc; }
    ++e->param_version;

    PopartArgs a;
    memset(&a, 0, sizeof a);
    a.rows = pl.rows;
    a.gamma = args->gamma; a.tau = args->tau; a.actor_lr = args->actor_lr; a.critic_lr = args->critic_lr; a.upper_lr = args->upper_lr;
    a.beta = args->beta;
    a.p0 = 0; a.p_count = P;
    const int ns = pl.ns;
    if (pl.dev_idx) {
        LearnArgs la;
        memset(&la, 0, sizeof la);
        la.batch = pl.rows; la.size = pl.min_size; la.device_rng = 1; la.rng_counter = e->rng_counter++; la.p0 = 0; la.p_count = P;
        prof_begin(e, PK_DRAW);
        hipLaunchKernelGGL(draw_kernel, dim3(P), dim3(256), pl.draw.lds_bytes, e->stream, e->d, la, pl.draw.flag);
        prof_end(e);
    }
    const dim3 blk(256), grid(((P + 7) / 8) * 8 * ns);
    prof_begin(e, PK_GRAD_CRITIC);
    hipLaunchKernelGGL(popart_target_kernel, grid, blk, e->lds_bytes, e->stream, e->d, a, ns);
    hipLaunchKernelGGL(popart_critic_kernel, grid, blk, e->lds_bytes, e->stream, e->d, a, ns);
    prof_end(e);
    a.stage = 0;
    prof_begin(e, PK_ADAM_CRITIC);
    hipLaunchKernelGGL(popart_step_kernel, dim3(P), blk, 0, e->stream, e->d, a, ns);
    prof_end(e);
    prof_begin(e, PK_GRAD_ACTOR);
    hipLaunchKernelGGL(popart_actor_kernel, grid, blk, e->lds_bytes, e->stream, e->d, a, ns);
    prof_end(e);
    a.stage = 1;
    prof_begin(e, PK_ADAM_ACTOR);
    hipLaunchKernelGGL(popart_step_kernel, dim3(P), blk, 0, e->stream, e->d, a, ns);
    prof_end(e);
    HIP_TRY(hipGetLastError());
    if (!args->out) return FRL_OK;
    HIP_TRY(hipMemcpyAsync(args->out, h.popart_out, (size_t)P * kPopartOut * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return FRL_OK;
}
