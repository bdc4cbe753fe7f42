// frl_envelope_learn (include/freerl_hip.h): ENVELOPE.learn (ENVELOPE_MORL_file/ENVELOPE_DQN.py:204-255) for a population, and the part
// of it that frl_envelope_ddpg_learn (frl_api_envelope_ddpg.inc) shares.  Included by frl_api.hip.
//
// Launch chain: [draw_kernel: `batch` distinct ring rows per learner when idx is NULL] -> envelope_weights_kernel (one workgroup per
// learner: the batch's rows expanded to batch x weight_num index entries, the preference vectors drawn when weights is NULL) ->
// envelope_grad_kernel (row chunks over the batch x weight_num rows) -> reduce + Adam + soft update (launch_adam: net 0, statistics
// in the actor slots, no clipping — the reference's clip_grad_norm_ runs between zero_grad() and backward(), on gradients that are None).

// Both envelope entry points up to and including envelope_weights_kernel: the plan (learn_plan.hpp: plan_envelope — `scalars`, named in
// `scalar_names`, are refused when NaN), then the staged rows, idx and the preference vectors on the device, the draw.
struct EnvelopeLaunch {
    EnvelopeArgs a;
    int rows, ns;                   // batch x weight_num; workgroups (= slabs) per learner
};
static int envelope_prelude(frl_engine* e, const EnvelopeCall& c, std::initializer_list<float> scalars, const char* scalar_names, EnvelopeLaunch* out) {
    const EngineDesc& h = e->h;
    const int B = c.batch, W = c.weight_num, RD = h.reward_dim, P = h.P;
    e->knobs = learn_knobs();
    EnvelopePlan pl;
    std::string why;
    if (const int rc = plan_envelope(h, e->size.data(), c, scalars, scalar_names, &pl, &e->idx_narrow, &why)) return fail(rc, "%s", why.c_str());
    int rc = flush_stage(e);
    if (rc) return rc;
    if (c.idx) { rc = upload_idx(e, e->idx_narrow, 1, B); if (rc) return rc; }
    const size_t wpitch = (size_t)h.batch_max * RD, wn = (size_t)W * RD;
    if (c.weights) {
        HIP_TRY(hipStreamSynchronize(e->stream));                       // pinned staging reuse
        for (int p = 0; p < P; ++p) {
            memcpy(e->h_env_w + p * wpitch, c.weights + p * wn, wn * sizeof(float));
            HIP_TRY(hipMemcpyAsync(h.env_w + p * wpitch, e->h_env_w + p * wpitch, wn * sizeof(float), hipMemcpyHostToDevice, e->stream));
        }
    }
    EnvelopeArgs& a = out->a;
    memset(&a, 0, sizeof a);
    a.batch = B; a.weight_num = W; a.draw_w = c.weights ? 0 : 1;
    a.gamma = c.gamma; a.beta = c.beta;
    a.p0 = 0; a.p_count = P;
    ++e->param_version;
    out->rows = pl.rows;
    out->ns = pl.ns;
    if (pl.dev_idx) {
        LearnArgs la;
        memset(&la, 0, sizeof la);
        la.batch = B; la.size = pl.min_size; la.device_rng = 1; la.rng_counter = e->rng_counter++; la.p0 = 0; la.p_count = P;
        prof_begin(e, PK_DRAW);
        hipLaunchKernelGGL(draw_kernel, dim3(P), dim3(256), pl.draw.lds_bytes, e->stream, e->d, la, pl.draw.flag);
        prof_end(e);
    }
    a.rng_counter = e->rng_counter++;
    hipLaunchKernelGGL(envelope_weights_kernel, dim3(P), dim3(256), 0, e->stream, e->d, a);
    return FRL_OK;
}

extern "C" int frl_envelope_learn(frl_engine* e, const frl_envelope_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_ENVELOPE_DQN) return wrong_engine(h, "frl_envelope_learn");
    EnvelopeLaunch L;
    if (const int rc = envelope_prelude(e, {args->batch, args->weight_num, args->gamma, args->beta, args->idx, args->weights},
                                        {args->gamma, args->tau, args->lr, args->beta}, "gamma / tau / lr / beta", &L)) return rc;
    AdamArgs ad{};
    ad.which = 1;                                  // net 0, statistics in the actor slots
    ad.batch = L.rows;                             // the loss partials are per row: beta d^2 + (1 - beta) / R sum_k e_k^2
    ad.lr = args->lr; ad.eps = 1e-8f; ad.beta1 = 0.9f; ad.beta2 = 0.999f;
    ad.clip = 0.f; ad.soft = 1; ad.tau = args->tau;
    launch_rowchunk_update(e, e->stream, h.P, 0, L.ns, ad, envelope_grad_kernel, L.a);
    HIP_TRY(hipGetLastError());
    if (!args->loss_out && !args->weights_out) return FRL_OK;
    return read_back(e, args->weights_out, args->weight_num, {ST_ACTOR_LOSS, args->loss_out});
}
