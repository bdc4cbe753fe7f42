// frl_envelope_ddpg_learn (include/freerl_hip.h): ENVELOPE_DDPG.learn (ENVELOPE_MORL_file/ENVELOPE_DDPG.py:254-320) for a population.
// Included by frl_api.hip.
//
// Launch chain: [draw_kernel: `batch` distinct ring rows per learner when idx is NULL] -> envelope_weights_kernel (the batch's rows
// expanded to batch x weight_num index entries, the preference vectors drawn when weights is NULL) -> envelope_ddpg_critic_kernel ->
// reduce + clip 0.5 + Adam of the critic (net 1) -> envelope_ddpg_actor_kernel (through the critic just stepped) -> reduce + clip 0.5
// + Adam of the actor (net 0).  Each Adam launch carries its net's soft update, as the DDPG launcher folds it: the reference moves
// both targets after both steps (:308-320), but the actor step reads the ONLINE critic only and leaves it alone, and nothing reads
// actor_target, so the targets end where the reference's do.

extern "C" int frl_envelope_ddpg_learn(frl_engine* e, const frl_envelope_ddpg_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo == ALGO_ENVELOPE_DQN) return fail(FRL_ERR_STATE, "frl_envelope_ddpg_learn on an envelope DQN engine (updates: frl_envelope_learn)");
    if (h.algo != ALGO_ENVELOPE_DDPG) return fail(FRL_ERR_STATE, "frl_envelope_ddpg_learn on an engine of algo %d", h.algo);
    const int B = args->batch, W = args->weight_num, RD = h.reward_dim, P = h.P;
    if (B < 1) return fail(FRL_ERR_INVALID, "batch %d must be >= 1", B);
    if (W < 1) return fail(FRL_ERR_INVALID, "weight_num %d must be >= 1", W);
    if ((long long)B * W > h.batch_max) return fail(FRL_ERR_INVALID, "batch %d x weight_num %d = %lld rows > batch_max %d", B, W, (long long)B * W, h.batch_max);
    if (!(args->gamma == args->gamma) || !(args->tau == args->tau) || !(args->actor_lr == args->actor_lr) || !(args->critic_lr == args->critic_lr) ||
        !(args->beta == args->beta))
        return fail(FRL_ERR_INVALID, "gamma / tau / actor_lr / critic_lr / beta is NaN");
    if (args->beta < 0.f || args->beta > 1.f) return fail(FRL_ERR_INVALID, "beta %g outside [0, 1]", (double)args->beta);
    int min_size = h.capacity;
    for (int p = 0; p < P; ++p) min_size = std::min(min_size, e->size[p]);
    if (min_size < B) return fail(FRL_ERR_STATE, "a ring holds %d rows < batch %d", min_size, B);
    const bool dev_idx = args->idx == nullptr;
    const bool table = B > 256 && 4 * B <= kDrawTableHost;
    const size_t draw_lds = ((size_t)2 * ((B + 3) & ~3) + (table ? 2 * kDrawTableHost : 0)) * sizeof(int);
    if (dev_idx && min_size < 2 * B) return fail(FRL_ERR_STATE, "device index draw needs len(buffer) >= 2*batch (have %d); pass idx", min_size);
    if (dev_idx && draw_lds > (size_t)(2 * 2048 + 2 * kDrawTableHost) * sizeof(int))
        return fail(FRL_ERR_INVALID, "device index draw of %d rows does not fit the draw kernel's LDS; pass idx", B);
    int rc = flush_stage(e);
    if (rc) return rc;
    rc = upload_idx_noise(e, args->idx, nullptr, B, 1);
    if (rc) return rc;
    const size_t wpitch = (size_t)h.batch_max * RD, wn = (size_t)W * RD;
    if (args->weights) {
        HIP_TRY(hipStreamSynchronize(e->stream));                       // pinned staging reuse
        for (int p = 0; p < P; ++p) {
            memcpy(e->h_env_w + p * wpitch, args->weights + p * wn, wn * sizeof(float));
            HIP_TRY(hipMemcpyAsync(h.env_w + p * wpitch, e->h_env_w + p * wpitch, wn * sizeof(float), hipMemcpyHostToDevice, e->stream));
        }
    }
    EnvelopeArgs a;
    memset(&a, 0, sizeof a);
    a.batch = B; a.weight_num = W; a.draw_w = args->weights ? 0 : 1;
    a.gamma = args->gamma; a.beta = args->beta;
    a.p0 = 0; a.p_count = P;
    ++e->param_version;
    const int rows = B * W;
    const int ns = ((rows + h.rc - 1) / h.rc + h.cps - 1) / h.cps;      // workgroups (= slabs) per learner
    const dim3 grid_chunks(((P + 7) / 8) * 8 * ns), grid_adam(P * h.Gmax);
    if (dev_idx) {
        LearnArgs la;
        memset(&la, 0, sizeof la);
        la.batch = B; la.size = min_size; la.device_rng = 1; la.rng_counter = e->rng_counter++; la.p0 = 0; la.p_count = P;
        prof_begin(e, PK_DRAW);
        hipLaunchKernelGGL(draw_kernel, dim3(P), dim3(256), draw_lds, e->stream, e->d, la, table ? 0 : 2);
        prof_end(e);
    }
    a.rng_counter = e->rng_counter++;
    hipLaunchKernelGGL(envelope_weights_kernel, dim3(P), dim3(256), 0, e->stream, e->d, a);
    AdamArgs ad;
    memset(&ad, 0, sizeof ad);
    ad.ns = ns; ad.batch = rows;                   // the loss partials are per row
    ad.eps = 1e-8f; ad.beta1 = 0.9f; ad.beta2 = 0.999f;
    ad.clip = 0.5f; ad.soft = 1; ad.tau = args->tau; ad.p0 = 0; ad.G = h.Gmax;
    prof_begin(e, PK_GRAD_CRITIC);
    hipLaunchKernelGGL(envelope_ddpg_critic_kernel, grid_chunks, dim3(256), e->lds_bytes, e->stream, e->d, a, ns);
    prof_end(e);
    ad.which = 0; ad.lr = args->critic_lr;         // net 1: beta d^2 + (1 - beta) / R sum_k e_k^2 per row
    prof_begin(e, PK_ADAM_CRITIC);
    launch_adam(e, e->stream, ad, P, grid_adam);
    prof_end(e);
    prof_begin(e, PK_GRAD_ACTOR);
    hipLaunchKernelGGL(envelope_ddpg_actor_kernel, grid_chunks, dim3(256), e->lds_bytes, e->stream, e->d, a, ns);
    prof_end(e);
    ad.which = 1; ad.lr = args->actor_lr;          // net 0: -sum_k Q_k / R per row
    prof_begin(e, PK_ADAM_ACTOR);
    launch_adam(e, e->stream, ad, P, grid_adam);
    prof_end(e);
    HIP_TRY(hipGetLastError());
    if (!args->critic_loss_out && !args->actor_loss_out && !args->weights_out) return FRL_OK;
    if (args->weights_out)
        for (int p = 0; p < P; ++p)
            HIP_TRY(hipMemcpyAsync(args->weights_out + p * wn, h.env_w + p * wpitch, wn * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    std::vector<float> st;
    if (args->critic_loss_out || args->actor_loss_out) {
        st.resize((size_t)P * ST_COUNT);
        HIP_TRY(hipMemcpyAsync(st.data(), h.stats, st.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int p = 0; p < P; ++p) {
        if (args->critic_loss_out) args->critic_loss_out[p] = st[(size_t)p * ST_COUNT + ST_CRITIC_LOSS];
        if (args->actor_loss_out) args->actor_loss_out[p] = st[(size_t)p * ST_COUNT + ST_ACTOR_LOSS];
    }
    return FRL_OK;
}
