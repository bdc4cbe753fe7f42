// frl_her_relabel (include/freerl_hip.h): the hindsight relabelling DDPG_simple_try_HER.py runs at an episode's end (:421-428), for
// every listed learner in one launch of her_relabel_kernel.  Included by frl_api.hip.
//
// Everything about which rows are read and written, and every refusal that concerns an episode, comes from her_plan.h.  The call's small
// arrays travel in ONE block: [weights G doubles | episodes n x HER_EP_INTS ints | picks | env_actions], pinned, one H2D copy.

extern "C" int frl_her_relabel(frl_engine* e, const frl_her_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    const frl_her_args& x = *args;
    if (h.algo != ALGO_DDPG && h.algo != ALGO_TD3 && h.algo != ALGO_SAC) return wrong_engine(h, "frl_her_relabel");
    if (e->per_on)       // priorities are assigned by add (PER_Buffer.add): rows written in place would leave the trees without them
        return fail(FRL_ERR_STATE, "frl_her_relabel bypasses the priority trees: a prioritised engine takes relabelled rows through frl_buffer_add_batch");
    const int P = h.P, n = x.n_episodes, A = h.rec.act_dim[0];
    if (n < 1 || n > P || n > 65535)               // (one grid row per episode)
        return fail(FRL_ERR_INVALID, "frl_her_relabel: %d episodes outside [1, min(n_learners = %d, 65535)]", n, P);
    if (!x.learners || !x.lengths) return fail(FRL_ERR_INVALID, "frl_her_relabel: learners / lengths is NULL");
    const HerShape shape{h.rec.obs_dim[0], x.state_dim, x.goal_dim, x.sample_num, x.sample_range};
    HerRefusal why = her_check_shape(shape);
    if (why != HER_OK)
        return fail(FRL_ERR_INVALID, "frl_her_relabel: %s (state_dim %d, goal_dim %d, obs_dim %d, sample_num %d, sample_range %d)", her_refusal_text(why),
                    x.state_dim, x.goal_dim, shape.obs_dim, x.sample_num, x.sample_range);
    if (x.mode != FRL_HER_SPARSE && x.mode != FRL_HER_SHAPING) return fail(FRL_ERR_INVALID, "frl_her_relabel: mode %d is no frl_her_mode", x.mode);
    if (!(x.tolerance == x.tolerance)) return fail(FRL_ERR_INVALID, "frl_her_relabel: tolerance is NaN");
    if (!x.weights && x.goal_dim != 3) return fail(FRL_ERR_INVALID, "frl_her_relabel: weights is NULL and goal_dim is %d: the script's weights are three", x.goal_dim);
    const int G = x.goal_dim;

    // staged adds first: the episode's rows must be in the ring, and the cursors below are what Buffer.add left
    int rc = flush_stage(e);
    if (rc) return rc;
    struct Episode { HerPlan pl; long long rows; };      // planned once per episode, from the cursor before the call
    std::vector<Episode> eps((size_t)n);
    std::vector<char> listed((size_t)P, 0);
    long long sum_L = 0, sum_rows = 0, max_rows = 0;
    for (int k = 0; k < n; ++k) {
        const int p = x.learners[k], L = x.lengths[k];
        if (p < 0 || p >= P) return fail(FRL_ERR_INVALID, "frl_her_relabel: learner %d out of range", p);
        if (listed[p]) return fail(FRL_ERR_INVALID, "frl_her_relabel: learner %d is listed twice (one episode per learner and call)", p);
        listed[p] = 1;
        why = her_check_episode(shape, h.capacity, e->size[p], L);
        if (why != HER_OK)
            return fail(why == HER_EPISODE_NOT_STORED ? FRL_ERR_STATE : FRL_ERR_INVALID, "frl_her_relabel: learner %d, L = %d: %s (stored rows %d, capacity %d)", p, L,
                        her_refusal_text(why), e->size[p], h.capacity);
        eps[k].pl = her_plan(h.capacity, e->index[p], L, x.sample_num, x.sample_range);
        const long long rows = eps[k].rows = her_total(eps[k].pl);
        sum_L += L; sum_rows += rows; max_rows = std::max(max_rows, rows);
    }
    if (sum_rows > 0x7fffffffll || sum_L > 0x7fffffffll) return fail(FRL_ERR_INVALID, "frl_her_relabel: %lld rows in one call", sum_rows);
    if (x.picks) {                                   // every injected offset inside its transition's candidates
        const int32_t* pk = x.picks;
        for (int k = 0; k < n; ++k) {
            const HerPlan& pl = eps[k].pl;
            for (int i = 0; i < pl.L; ++i)
                for (int s = 0, ni = her_n(pl, i); s < ni; ++s, ++pk)
                    if (*pk < 0 || *pk >= her_m(pl, i))
                        return fail(FRL_ERR_INVALID, "frl_her_relabel: learner %d, transition %d: pick %d outside [0, %d)", x.learners[k], i, (int)*pk, her_m(pl, i));
        }
    }

    // the one block
    const size_t w_bytes = (size_t)G * sizeof(double), ep_bytes = (size_t)n * HER_EP_INTS * sizeof(int);
    const size_t pk_bytes = x.picks ? (size_t)sum_rows * sizeof(int) : 0, act_bytes = x.env_actions ? (size_t)sum_L * A * sizeof(float) : 0;
    const size_t bytes = w_bytes + ep_bytes + pk_bytes + act_bytes;
    // The event guards the PINNED block: the previous call's copy may still be reading it.  The device block needs no guard of its own:
    // a copy into it is ordered behind the previous launch on the stream, and growing it frees the old block with hipFree, which
    // waits for the device (HipMem::device_free) - so no launch is still reading what is freed.
    if (e->her_inflight) {
        HIP_TRY(hipEventSynchronize(e->ev_her));
        e->her_inflight = false;
    }
    if (!e->ev_her) HIP_TRY(hipEventCreateWithFlags(&e->ev_her, hipEventDisableTiming));
    HIP_TRY(e->mem.grow(&e->h_her, e->her_cap_h, bytes, MEM_PINNED));
    HIP_TRY(e->mem.grow(&e->d_her, e->her_cap_d, bytes, MEM_DEVICE));
    double* hw = reinterpret_cast<double*>(e->h_her);
    int* hep = reinterpret_cast<int*>(e->h_her + w_bytes);
    static const double script_w[3] = {1.0, 1.0, 0.1};      // :254
    memcpy(hw, x.weights ? x.weights : script_w, w_bytes);
    long long pick0 = 0, act0 = 0;
    for (int k = 0; k < n; ++k) {
        const HerPlan& pl = eps[k].pl;
        int* q = hep + (size_t)k * HER_EP_INTS;
        q[HER_EP_LEARNER] = x.learners[k]; q[HER_EP_L] = pl.L; q[HER_EP_CURSOR] = pl.cursor; q[HER_EP_PICK0] = (int)pick0; q[HER_EP_ACT0] = (int)act0;
        pick0 += eps[k].rows;
        act0 += pl.L;
    }
    if (pk_bytes) memcpy(e->h_her + w_bytes + ep_bytes, x.picks, pk_bytes);
    if (act_bytes) memcpy(e->h_her + w_bytes + ep_bytes + pk_bytes, x.env_actions, act_bytes);
    HIP_TRY(hipMemcpyAsync(e->d_her, e->h_her, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_her, e->stream));
    e->her_inflight = true;

    HerArgs a;
    memset(&a, 0, sizeof a);
    a.weights = reinterpret_cast<const double*>(e->d_her);
    a.eps = reinterpret_cast<const int*>(e->d_her + w_bytes);
    a.picks = pk_bytes ? reinterpret_cast<const int*>(e->d_her + w_bytes + ep_bytes) : nullptr;
    a.env_actions = act_bytes ? reinterpret_cast<const float*>(e->d_her + w_bytes + ep_bytes + pk_bytes) : nullptr;
    a.tolerance = x.tolerance;
    a.capacity = h.capacity; a.S = x.state_dim; a.G = G; a.A = A;
    a.sample_num = x.sample_num; a.sample_range = x.sample_range; a.mode = x.mode;
    a.counter = x.picks ? 0 : e->her_calls++;
    a.seed = h.seed;
    const int groups_per_block = 256 / 16;
    hipLaunchKernelGGL(her_relabel_kernel, dim3((unsigned)((max_rows + groups_per_block - 1) / groups_per_block), (unsigned)n), dim3(256), 0, e->stream,
                       h.replay, h.rec, a);
    HIP_TRY(hipGetLastError());

    // the cursors, as `rows` calls of Buffer.add would leave them (Buffer.py:36-38)
    for (int k = 0; k < n; ++k) {
        const int p = x.learners[k];
        e->index[p] = her_dst(eps[k].pl, eps[k].rows);   // the row behind the last one written
        e->size[p] = (int)std::min<long long>(e->size[p] + eps[k].rows, h.capacity);
        if (x.rows_out) x.rows_out[k] = (int)eps[k].rows;
    }
    e->size_flushed = e->size;
    return FRL_OK;
}
