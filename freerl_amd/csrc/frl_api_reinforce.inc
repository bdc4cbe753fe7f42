// frl_reinforce_learn (include/freerl_hip.h): REINFORCE.learn (REINFORCE_file/REINFORCE.py:104-127) for a population whose learners
// bring episodes of different lengths, or none.  Included by frl_api.hip.
//
// Launch chain: reinforce_returns_kernel (one workgroup per learner) -> reinforce_grad_kernel (row chunks of CONSECUTIVE ring rows,
// the grid sized for the longest episode of the call) -> reduce + Adam (launch_adam with AdamArgs::ragged).  The learners' row
// counts travel in EngineDesc::ep_n; every workgroup of the three launches that belongs to a learner with no rows returns at once.

extern "C" int frl_reinforce_learn(frl_engine* e, const frl_reinforce_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_REINFORCE) return wrong_engine(h, "frl_reinforce_learn");
    if (!(args->gamma == args->gamma) || !(args->lr == args->lr)) return fail(FRL_ERR_INVALID, "gamma / lr is NaN");
    const int P = h.P;
    int n_max = 0;
    for (int p = 0; p < P; ++p) {
        const int n = args->n_steps ? args->n_steps[p] : e->size[p];
        if (n < 0 || n > h.capacity) return fail(FRL_ERR_INVALID, "learner %d: %d steps outside [0, capacity = %d]", p, n, h.capacity);
        if (n == 1)
            return fail(FRL_ERR_INVALID, "learner %d has exactly one stored step: the std of one return is NaN "
                                         "(the reference turns every parameter into NaN here)", p);
        if (n > e->size[p]) return fail(FRL_ERR_STATE, "learner %d: %d steps asked for, its ring holds %d", p, n, e->size[p]);
        if (n > 0 && e->index[p] != e->size[p] % h.capacity)      // rows 0..n-1 are in time order only in a ring filled from an empty cursor
            return fail(FRL_ERR_STATE, "learner %d: ring cursor (%d, %d) was not filled from empty: its rows are not in time order", p, e->index[p], e->size[p]);
        n_max = std::max(n_max, n);
    }
    if (n_max == 0) return FRL_OK;                 // every learner sits out
    int rc = flush_stage(e);
    if (rc) return rc;
    const unsigned slot = e->ep_seq++ & 1u;
    int* hn = e->h_ep_n + (size_t)slot * P;
    if (e->ep_seq > 2) HIP_TRY(hipEventSynchronize(e->ev_ep[slot]));     // the copy out of this slot two calls ago
    for (int p = 0; p < P; ++p) hn[p] = args->n_steps ? args->n_steps[p] : e->size[p];
    HIP_TRY(hipMemcpyAsync(h.ep_n, hn, (size_t)P * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_ep[slot], e->stream));
    ++e->param_version;

    const int ns = rowchunk_ns(h, n_max);          // workgroups (= slabs) of the longest episode
    prof_begin(e, PK_DRAW);
    hipLaunchKernelGGL(reinforce_returns_kernel, dim3(P), dim3(256), 0, e->stream, e->d, args->gamma);
    prof_end(e);
    AdamArgs ad{};
    ad.which = 1;                                  // net 0, statistics in the actor slots
    ad.ragged = 1;
    ad.batch = 1;                                  // the loss is a sum
    ad.lr = args->lr; ad.eps = args->adam_eps > 0 ? args->adam_eps : 1e-8f; ad.beta1 = 0.9f; ad.beta2 = 0.999f;
    ad.clip = 0.f;
    launch_rowchunk_update(e, e->stream, P, 0, ns, ad, reinforce_grad_kernel, 0, P);
    HIP_TRY(hipGetLastError());
    for (int p = 0; p < P; ++p)
        if (hn[p] > 0) { e->index[p] = 0; e->size[p] = 0; }              // self.rewards = [] ... (:125-127)
    e->size_flushed = e->size;
    if (!args->loss_out && !args->returns_out) return FRL_OK;
    if (args->returns_out)
        for (int p = 0; p < P; ++p)
            if (hn[p] > 0)
                HIP_TRY(hipMemcpyAsync(args->returns_out + (size_t)p * h.capacity, h.isw + (size_t)p * h.batch_max, (size_t)hn[p] * sizeof(float),
                                       hipMemcpyDeviceToHost, e->stream));
    return read_back(e, nullptr, 0, {ST_ACTOR_LOSS, args->loss_out}, {0, nullptr}, hn);
}
