// frl_envelope_learn (include/freerl_hip.h): ENVELOPE.learn (ENVELOPE_MORL_file/ENVELOPE_DQN.py:204-255) for a population, and the part
// of it that frl_envelope_ddpg_learn (frl_api_envelope_ddpg.inc) shares.  Included by frl_api.hip.
//
// Launch chain: [draw_kernel: `batch` distinct ring rows per learner when idx is NULL] -> envelope_weights_kernel (one workgroup per
// learner: the batch's rows expanded to batch x weight_num index entries, the preference vectors drawn when weights is NULL) ->
// envelope_grad_kernel (row chunks over the batch x weight_num rows) -> reduce + Adam + soft update (launch_adam: net 0, statistics
// in the actor slots, no clipping — the reference's clip_grad_norm_ runs between zero_grad() and backward(), on gradients that are None).

// Both envelope entry points up to and including envelope_weights_kernel: validation, the staged rows, idx and the preference vectors
// on the device, the draw.  `scalars` (named in `scalar_names`) are refused when NaN.
struct EnvelopeCall {
    int batch, weight_num;
    float gamma, beta;
    const int64_t* idx;
    const float* weights;
};
struct EnvelopeLaunch {
    EnvelopeArgs a;
    int rows, ns;                   // batch x weight_num; workgroups (= slabs) per learner
};
static int envelope_prelude(frl_engine* e, const EnvelopeCall& c, std::initializer_list<float> scalars, const char* scalar_names, EnvelopeLaunch* out) {
    const EngineDesc& h = e->h;
    const int B = c.batch, W = c.weight_num, RD = h.reward_dim, P = h.P;
    if (B < 1) return fail(FRL_ERR_INVALID, "batch %d must be >= 1", B);
    if (W < 1) return fail(FRL_ERR_INVALID, "weight_num %d must be >= 1", W);
    if ((long long)B * W > h.batch_max) return fail(FRL_ERR_INVALID, "batch %d x weight_num %d = %lld rows > batch_max %d", B, W, (long long)B * W, h.batch_max);
    for (const float v : scalars)
        if (!(v == v)) return fail(FRL_ERR_INVALID, "%s is NaN", scalar_names);
    if (c.beta < 0.f || c.beta > 1.f) return fail(FRL_ERR_INVALID, "beta %g outside [0, 1]", (double)c.beta);
    int min_size = h.capacity;
    for (int p = 0; p < P; ++p) min_size = std::min(min_size, e->size[p]);
    if (min_size < B) return fail(FRL_ERR_STATE, "a ring holds %d rows < batch %d", min_size, B);
    const bool dev_idx = c.idx == nullptr;
    const bool table = B > 256 && 4 * B <= kDrawTableHost;
    const size_t draw_lds = ((size_t)2 * ((B + 3) & ~3) + (table ? 2 * kDrawTableHost : 0)) * sizeof(int);
    if (dev_idx && min_size < 2 * B) return fail(FRL_ERR_STATE, "device index draw needs len(buffer) >= 2*batch (have %d); pass idx", min_size);
    if (dev_idx && draw_lds > (size_t)(2 * 2048 + 2 * kDrawTableHost) * sizeof(int))
        return fail(FRL_ERR_INVALID, "device index draw of %d rows does not fit the draw kernel's LDS; pass idx", B);
    int rc = flush_stage(e);
    if (rc) return rc;
    rc = upload_idx_noise(e, c.idx, nullptr, B, 1);
    if (rc) return rc;
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
    out->rows = B * W;
    out->ns = rowchunk_ns(h, out->rows);
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
