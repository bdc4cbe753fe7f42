// frl_cem_gd3pg_learn and the ring entry points (include/freerl_hip.h): CEM_GD3PG.learn (CEM_GD3PG_file/CEM_GD3PG.py:160-231) for a
// population.  Included by frl_api.hip.
//
// Launch chain: [cem_draw_kernel: both halves below ring 1's size when idx is NULL] -> cem_critic_kernel (TD targets from both target
// actors, the critic's gradient, the guided actor's sum c^2) -> cem_step_kernel (critic: reduce + clip 0.5 + Adam + soft update) ->
// cem_actor_kernel (units (learner, actor), through the critic just stepped) -> cem_step_kernel (both actors).  The reference moves the
// three targets after all three steps (:218-231); no step reads a target that an earlier step of the same call has moved, so folding each
// soft update into its net's step ends where the reference does.

// ---- the rings of a learner (ring 0 everywhere; ring 1 on FRL_ALGO_CEM_GD3PG engines)
extern "C" int frl_ring_add(frl_engine* e, int learner, int ring, const float* record) {
    ENG(e);
    if (!record) return fail(FRL_ERR_INVALID, "record is NULL");
    return stage_one(e, learner, record, ring);
}

extern "C" int frl_ring_add_batch(frl_engine* e, int ring, int n, const int* learners, const float* records) {
    ENG(e);
    if (n < 0 || (n > 0 && !records)) return fail(FRL_ERR_INVALID, "bad batch");
    const int w = e->h.rec.width;
    for (int i = 0; i < n; ++i)
        if (const int rc = stage_one(e, learners ? learners[i] : 0, records + (size_t)i * w, ring)) return rc;
    return FRL_OK;
}

static int ring_check(const frl_engine* e, int learner, int ring) {
    if (learner < 0 || learner >= e->h.P) return fail(FRL_ERR_INVALID, "learner out of range");
    if (ring < 0 || ring >= e->n_rings) return fail(FRL_ERR_INVALID, "ring %d out of range (the engine has %d per learner)", ring, e->n_rings);
    return FRL_OK;
}

extern "C" int frl_ring_cursor_get(const frl_engine* e, int learner, int ring, int* index_out, int* size_out) {
    if (!e) return fail(FRL_ERR_INVALID, "engine is NULL");
    if (const int rc = ring_check(e, learner, ring)) return rc;
    const size_t cur = (size_t)ring * e->h.P + learner;
    if (index_out) *index_out = e->index[cur];
    if (size_out) *size_out = e->size[cur];
    return FRL_OK;
}

extern "C" int frl_ring_cursor_set(frl_engine* e, int learner, int ring, int index, int size) {
    ENG(e);
    if (const int rc = ring_check(e, learner, ring)) return rc;
    if (index < 0 || index >= e->ring_cap || size < 0 || size > e->ring_cap)
        return fail(FRL_ERR_INVALID, "cursor (%d,%d) outside capacity %d", index, size, e->ring_cap);
    if (const int rc = flush_stage(e)) return rc;      // (as frl_buffer_cursor_set: a scatter launch may not hold a ring row twice)
    const size_t cur = (size_t)ring * e->h.P + learner;
    e->index[cur] = index;
    e->size[cur] = size;
    return FRL_OK;
}

// ---- learn
extern "C" int frl_cem_gd3pg_learn(frl_engine* e, const frl_cem_gd3pg_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_CEM_GD3PG) return wrong_engine(h, "frl_cem_gd3pg_learn");
    const int P = h.P, C = e->ring_cap;
    if (args->batch < 2) return fail(FRL_ERR_INVALID, "batch %d must be >= 2 (half of it comes from each ring)", args->batch);
    for (const float v : {args->gamma, args->tau, args->actor_lr, args->critic_lr, args->lambda})
        if (!(v == v)) return fail(FRL_ERR_INVALID, "gamma / tau / actor_lr / critic_lr / lambda is NaN");
    if (!args->f1_more || !args->delta) return fail(FRL_ERR_INVALID, "f1_more / delta is NULL (one entry per learner)");
    for (int p = 0; p < P; ++p)
        if (!(args->delta[p] == args->delta[p])) return fail(FRL_ERR_INVALID, "delta of learner %d is NaN", p);
    // sample() (:160-164): total = len(buffer_domain) bounds the batch AND both draws; the population shares one launch shape, so its
    // smallest ring 1 decides
    const int* size1 = e->size.data() + P;
    int min1 = C;
    for (int p = 0; p < P; ++p) min1 = std::min(min1, size1[p]);
    if (min1 < 2) {
        int who = 0;
        for (int p = 0; p < P; ++p) if (size1[p] == min1) { who = p; break; }
        return fail(FRL_ERR_STATE, "ring 1 (buffer_domain) of learner %d holds %d rows < 2: no half batch can be drawn from it", who, min1);
    }
    const int half = std::min(min1, args->batch) / 2, rows = 2 * half;
    if (rows > h.batch_max) return fail(FRL_ERR_INVALID, "2 x half = %d rows > batch_max %d", rows, h.batch_max);
    const size_t draw_lds = (size_t)2 * ((half + 3) & ~3) * sizeof(int);
    if (!args->idx && draw_lds > 64 * 1024) return fail(FRL_ERR_INVALID, "device index draw of 2 x %d rows does not fit the draw kernel's LDS; pass idx", half);
    if (args->idx) {
        HIP_TRY(hipStreamSynchronize(e->stream));                       // pinned scratch reuse
        for (int p = 0; p < P; ++p)
            for (int r = 0; r < 2; ++r) {
                const int64_t* src = args->idx + ((size_t)p * 2 + r) * half;
                int* dst = e->h_idx + idx_offset(h, p, 0, r * half);
                const int bound = r == 0 ? C : size1[p];      // ring 0: rows never written are zeros, as the reference's (:165-167)
                for (int i = 0; i < half; ++i) {
                    if (src[i] < 0 || src[i] >= bound)
                        return fail(FRL_ERR_INVALID, "learner %d: idx entry %lld of ring %d outside [0, %d) (%s)", p, (long long)src[i], r, bound,
                                    r == 0 ? "its capacity" : "the rows it holds");
                    dst[i] = (int)src[i] + r * C;
                }
            }
    }
    int rc = flush_stage(e);
    if (rc) return rc;
    if (args->idx) HIP_TRY(hipMemcpyAsync(h.idx, e->h_idx, e->idx_count * sizeof(int), hipMemcpyHostToDevice, e->stream));
    // is_F1_more and delta of every learner, staged in two alternating pinned slots (the call does not wait for the stream)
    const unsigned slot = e->ep_seq++ & 1u;
    float* hc = e->h_cem_ctl + (size_t)slot * 2 * P;
    if (e->ep_seq > 2) HIP_TRY(hipEventSynchronize(e->ev_ep[slot]));     // the copy out of this slot two calls ago
    for (int p = 0; p < P; ++p) { hc[p] = args->f1_more[p] ? 1.f : 0.f; hc[P + p] = args->delta[p]; }
    HIP_TRY(hipMemcpyAsync(h.cem_ctl, hc, (size_t)2 * P * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_ep[slot], e->stream));
    ++e->param_version;

    CemArgs a;
    memset(&a, 0, sizeof a);
    a.rows = rows; a.half = half; a.size1 = min1; a.ring_cap = C;
    a.gamma = args->gamma; a.lambda = args->lambda; a.tau = args->tau; a.actor_lr = args->actor_lr; a.critic_lr = args->critic_lr;
    a.p0 = 0; a.p_count = P;
    const int ns = rowchunk_ns(h, rows);
    if (!args->idx) {
        a.rng_counter = e->rng_counter++;
        prof_begin(e, PK_DRAW);
        hipLaunchKernelGGL(cem_draw_kernel, dim3(P), dim3(256), draw_lds, e->stream, e->d, a);
        prof_end(e);
    }
    const dim3 blk(256);
    prof_begin(e, PK_GRAD_CRITIC);
    hipLaunchKernelGGL(cem_critic_kernel, dim3(((P + 7) / 8) * 8 * ns), blk, e->lds_bytes, e->stream, e->d, a, ns);
    prof_end(e);
    a.stage = 0;
    prof_begin(e, PK_ADAM_CRITIC);
    hipLaunchKernelGGL(cem_step_kernel, dim3(P), blk, 0, e->stream, e->d, a, ns);
    prof_end(e);
    prof_begin(e, PK_GRAD_ACTOR);
    hipLaunchKernelGGL(cem_actor_kernel, dim3(((kCemActors * P + 7) / 8) * 8 * ns), blk, e->lds_bytes, e->stream, e->d, a, ns);
    prof_end(e);
    a.stage = 1;
    prof_begin(e, PK_ADAM_ACTOR);
    hipLaunchKernelGGL(cem_step_kernel, dim3(kCemActors * P), blk, 0, e->stream, e->d, a, ns);
    prof_end(e);
    HIP_TRY(hipGetLastError());
    if (!args->out) return FRL_OK;
    HIP_TRY(hipMemcpyAsync(args->out, h.cem_out, (size_t)P * 8 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return FRL_OK;
}
