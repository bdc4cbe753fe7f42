// MAPPO / IPPO entry points (included at the end of frl_api.hip); mappo_learn_chain is frl_happo_learn's too (frl_api_happo.inc).

extern "C" int frl_net_norm_set(frl_engine* e, int feature_norm, int layer_norm) {
    ENG(e);
    if (!is_mappo_family(e->h.algo)) return wrong_engine(e->h, "frl_net_norm_set");
    e->h.feature_norm = feature_norm ? 1 : 0;
    e->h.layer_norm = layer_norm ? 1 : 0;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->d, &e->h, sizeof e->h, hipMemcpyHostToDevice));
    return FRL_OK;
}

// MAPPO_for_mask_action.py on a FRL_ALGO_MAPPO engine: the record column of the first mask block (behind the log-prob and adv_done
// columns), copied to the device like frl_net_norm_set's flags
extern "C" int frl_action_mask_set(frl_engine* e, int on) {
    ENG(e);
    if (e->h.algo != FRL_ALGO_MAPPO) return wrong_engine(e->h, "frl_action_mask_set");
    const RecordDesc& R = e->h.rec;
    if (!e->h.n_discrete) return fail(FRL_ERR_INVALID, "frl_action_mask_set: the engine's actions are continuous (a mask closes discrete actions)");
    int blocks = 0;
    for (int i = 0; i < e->h.n_agents; ++i) blocks += e->h.net[2 * i].L[2].n;
    const int first = 2 * e->h.n_agents;      // one log-prob and one adv_done column per agent come first
    if (R.extra < first + blocks)
        return fail(FRL_ERR_INVALID, "frl_action_mask_set: extra_cols %d < %d log-prob and adv_done columns + %d mask columns", R.extra, first, blocks);
    if (R.extra < first + blocks + e->h.state_dim)      // the state block (frl_create_ex) is the last state_dim columns: the masks may not reach into it
        return fail(FRL_ERR_INVALID, "frl_action_mask_set: extra_cols %d < %d log-prob and adv_done columns + %d mask columns + %d state columns", R.extra, first,
                    blocks, e->h.state_dim);
    e->h.mask_off = on ? R.extra_off + first : 0;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->d, &e->h, sizeof e->h, hipMemcpyHostToDevice));
    return FRL_OK;
}

// select_action of a masked engine: one synchronous categorical draw per row of an actor, host in / host out
extern "C" int frl_act_masked(frl_engine* e, int net, int n_rows, int in_dim, const float* in_host, const float* mask_host, const float* eps_host,
                              float* out_host, float* logp_host) {
    ENG(e);
    if (e->h.algo != FRL_ALGO_MAPPO) return wrong_engine(e->h, "frl_act_masked");
    if (!e->h.mask_off) return fail(FRL_ERR_STATE, "frl_act_masked: action masking is off for this engine (frl_action_mask_set)");
    if (net < 0 || net >= e->h.n_nets || net % 2) return fail(FRL_ERR_INVALID, "net %d is not an actor (nets 0, 2, ..)", net);
    if (!in_host || !mask_host || !out_host || n_rows < 1) return fail(FRL_ERR_INVALID, "bad argument");
    const NetDesc& N = e->h.net[net];
    if (in_dim != N.L[0].k) return fail(FRL_ERR_INVALID, "in_dim %d != layer input %d", in_dim, N.L[0].k);
    const size_t rows = (size_t)e->h.P * n_rows, in_n = rows * in_dim, out_n = rows * N.L[2].n;
    int rc = act_scratch(e, in_n, 2 * out_n);      // the masks ride behind the draws
    if (rc) return rc;
    float* d_mask = e->d_act_eps + out_n;
    HIP_TRY(hipMemcpyAsync(e->d_act_in, in_host, in_n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_mask, mask_host, out_n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (eps_host) HIP_TRY(hipMemcpyAsync(e->d_act_eps, eps_host, out_n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    ActArgs a;
    memset(&a, 0, sizeof a);
    a.net = net; a.mode = ACTM_CAT_SAMPLE; a.n_rows = n_rows; a.in_dim = in_dim;
    a.in = e->d_act_in; a.eps = eps_host ? e->d_act_eps : nullptr; a.out = e->d_act_out; a.out_logp = logp_host ? e->d_act_logp : nullptr;
    a.device_eps = eps_host ? 0 : 1;
    if (!eps_host) a.rng_counter = e->rng_counter++;
    hipLaunchKernelGGL(mappo_mask_act_kernel, dim3((n_rows + e->h.rc - 1) / e->h.rc, e->h.P), dim3(256), e->lds_bytes, e->stream, e->d, a, (const float*)d_mask);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, e->d_act_out, rows * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (logp_host) HIP_TRY(hipMemcpyAsync(logp_host, e->d_act_logp, rows * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return FRL_OK;
}

// HAPPO's part of a call (frl_happo_learn): nullptr for frl_mappo_learn
struct HappoCall {
    const int32_t* agent_order;
    float* factor_out;
};

// the whole of frl_mappo_learn, and of frl_happo_learn with `hc`: the argument refusals, the permutations, the three advantage launches,
// then mappo_update_kernel once or happo_update_kernel once per visiting position, all on the engine's one stream
static int mappo_learn_chain(frl_engine* e, const frl_mappo_args* args, const HappoCall* hc) {
    const EngineDesc& h = e->h;
    const int T = args->horizon, mb = args->minibatch, K = args->k_epochs, n = h.n_agents;
    if (T < 2 || T > h.capacity) return fail(FRL_ERR_INVALID, "horizon %d outside [2, capacity %d]", T, h.capacity);
    if (mb < 1 || mb > h.batch_max) return fail(FRL_ERR_INVALID, "minibatch %d outside [1,%d]", mb, h.batch_max);
    if (K < 1) return fail(FRL_ERR_INVALID, "k_epochs must be >= 1");
    // a state engine with the reference's pairing (MAPPO_for_mask_action_state.py:371-373): torch.cat of obs_[index] with the unindexed
    // `state` raises unless the minibatch is the whole horizon
    if (h.state_dim > 0 && h.state_rows == FRL_STATE_ROWS_POSITION && mb != T)
        return fail(FRL_ERR_INVALID, "minibatch %d != horizon %d on an engine with FRL_STATE_ROWS_POSITION (the state block is taken by position in the one "
                                     "minibatch; FRL_STATE_ROWS_SAMPLE takes any minibatch)", mb, T);
    if (args->loss_kind != FRL_LOSS_MSE && args->loss_kind != FRL_LOSS_HUBER) return fail(FRL_ERR_INVALID, "loss_kind %d (FRL_LOSS_MSE or FRL_LOSS_HUBER)", args->loss_kind);
    if (args->loss_kind == FRL_LOSS_HUBER && !(args->huber_delta > 0.f)) return fail(FRL_ERR_INVALID, "FRL_LOSS_HUBER needs huber_delta > 0");
    const int n_mb = (T + mb - 1) / mb;
    const size_t P = h.P, U = P * n;
    std::vector<int> perm;
    if (args->perms) {
        perm.resize(U * (size_t)K * T);
        for (size_t i = 0; i < perm.size(); ++i) {
            const int64_t v = args->perms[i];
            if (v < 0 || v >= T) return fail(FRL_ERR_INVALID, "permutation entry %lld outside [0,%d)", (long long)v, T);
            perm[i] = (int)v;
        }
    }
    std::vector<int> order;
    if (hc && hc->agent_order) {
        order.assign(hc->agent_order, hc->agent_order + U);
        for (size_t p = 0; p < P; ++p) {
            unsigned seen = 0;
            for (int k = 0; k < n; ++k) {
                const int v = order[p * n + k];
                if (v < 0 || v >= n || (seen >> v & 1u)) return fail(FRL_ERR_INVALID, "agent_order of learner %d is not a permutation of 0..%d (entry %d: %d)", (int)p, n - 1, k, v);
                seen |= 1u << v;
            }
        }
    }
    int rc = flush_stage(e);
    if (rc) return rc;
    const size_t trace_n = U * (size_t)K * n_mb * 2;
    // (HAPPO: old [P][T] and factor [P][n][T] behind the trace, the visiting order [P][n] behind the permutations)
    HIP_TRY(e->mem.grow(&e->d_ppo, e->ppo_cap, 7 * U * T + trace_n + (hc ? (P + U) * T : 0), MEM_DEVICE));
    HIP_TRY(e->mem.grow(&e->d_perm, e->perm_cap, U * (size_t)K * T + (hc ? U : 0), MEM_DEVICE));
    // permutations: the caller's np.random.permutation draws, one per (agent, epoch) in agent-major order (MAPPO.py:391-395,
    // IPPO.py:254,275-277), else ppo_perm_kernel's with a unit = (learner, agent); horizons beyond 8192 rows: a host Fisher-Yates
    int Tpad = 2;
    while (Tpad < T) Tpad <<= 1;
    const bool dev_perm = !args->perms && Tpad <= 8192;
    if (dev_perm) {
        hipLaunchKernelGGL(ppo_perm_kernel, dim3(K, (unsigned)U), dim3(256), (size_t)Tpad * sizeof(unsigned long long), e->stream,
                           e->d_perm, T, Tpad, (unsigned long long)(++e->rng_counter), (unsigned long long)h.seed);
    } else {
        if (!args->perms) {
            perm.resize(U * (size_t)K * T);
            unsigned long long s = h.seed ^ (0xD1B54A32D192ED03ull * (++e->rng_counter));
            for (size_t blk = 0; blk < U * (size_t)K; ++blk) {
                int* q = perm.data() + blk * T;
                for (int i = 0; i < T; ++i) q[i] = i;
                for (int i = T - 1; i > 0; --i) std::swap(q[i], q[(int)(splitmix64(s) % (unsigned long long)(i + 1))]);
            }
        }
        HIP_TRY(hipMemcpyAsync(e->d_perm, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    MappoArgs a;
    memset(&a, 0, sizeof a);
    a.horizon = T; a.minibatch = mb; a.k_epochs = K; a.adv_norm = args->adv_norm ? 1 : 0;
    a.huber = args->loss_kind == FRL_LOSS_HUBER ? 1 : 0;
    a.huber_delta = args->huber_delta;
    a.gamma = args->gamma; a.lmbda = args->lmbda; a.clip = args->clip; a.ent_coef = args->ent_coef;
    a.actor_lr = args->actor_lr; a.critic_lr = args->critic_lr;
    a.adam_eps = args->adam_eps > 0 ? args->adam_eps : 1e-8f;
    a.beta1 = 0.9f; a.beta2 = 0.999f;
    a.clip_norm = args->clip_norm;
    float* q = e->d_ppo;
    a.td = q; q += U * T;
    a.advd = q; q += U * T;
    a.vs = q; q += U * T;
    a.adv_seq = q; q += U * T;
    a.adv_raw = q; q += U * T;
    a.adv = q; q += U * T;
    a.vtarget = q; q += U * T;
    a.trace = q;
    a.perm = e->d_perm;
    if (h.state_dim > 0)      // the critic's row from two segments (kernels_mappo_state.hip)
        hipLaunchKernelGGL(mappo_state_values_kernel, dim3((T + h.rc - 1) / h.rc, (unsigned)U), dim3(256), e->lds_bytes, e->stream, e->d, a);
    else
        hipLaunchKernelGGL(mappo_values_kernel, dim3((T + h.rc - 1) / h.rc, (unsigned)U), dim3(256), e->lds_bytes, e->stream, e->d, a);
    hipLaunchKernelGGL(gae_dense_kernel, dim3((unsigned)U), dim3(256), 0, e->stream, a.td, a.advd, T, args->gamma * args->lmbda, a.adv_seq);
    hipLaunchKernelGGL(mappo_adv_kernel, dim3(h.P), dim3(256), 0, e->stream, e->d, a);
    HappoArgs x = {};
    if (hc) {
        // the visiting order (HAPPO.py:375: torch.randperm(n)): the caller's, else a host Fisher-Yates per learner from the seed and counter
        if (order.empty()) {
            order.resize(U);
            unsigned long long s = h.seed ^ (0xD1B54A32D192ED03ull * (++e->rng_counter));
            for (size_t p = 0; p < P; ++p) {
                int* q = order.data() + p * n;
                for (int i = 0; i < n; ++i) q[i] = i;
                for (int i = n - 1; i > 0; --i) std::swap(q[i], q[(int)(splitmix64(s) % (unsigned long long)(i + 1))]);
            }
        }
        int* d_order = e->d_perm + U * (size_t)K * T;
        HIP_TRY(hipMemcpyAsync(d_order, order.data(), U * sizeof(int), hipMemcpyHostToDevice, e->stream));
        x.order = d_order;
        x.old = a.trace + trace_n;
        x.factor = x.old + P * T;
        for (x.k = 0; x.k < n; ++x.k)
            hipLaunchKernelGGL(happo_update_kernel, dim3((unsigned)P, 2), dim3(256), e->lds_bytes, e->stream, e->d, a, x);
    } else if (h.state_dim > 0) {      // the critics' rows with the state block behind the observations (kernels_mappo_state.hip)
        if (h.mask_off) hipLaunchKernelGGL(mappo_state_mask_update_kernel, dim3((unsigned)U, 2), dim3(256), e->lds_bytes, e->stream, e->d, a);
        else hipLaunchKernelGGL(mappo_state_update_kernel, dim3((unsigned)U, 2), dim3(256), e->lds_bytes, e->stream, e->d, a);
    } else if (h.mask_off) {      // the discrete actors' rows under their mask blocks (kernels_mappo_mask.hip)
        hipLaunchKernelGGL(mappo_mask_update_kernel, dim3((unsigned)U, 2), dim3(256), e->lds_bytes, e->stream, e->d, a);
    } else {
        hipLaunchKernelGGL(mappo_update_kernel, dim3((unsigned)U, 2), dim3(256), e->lds_bytes, e->stream, e->d, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));      // `perm` and `order` (pageable) must outlive their copies
    ++e->param_version;
    if (args->adv_out) HIP_TRY(hipMemcpy(args->adv_out, a.adv_raw, U * T * sizeof(float), hipMemcpyDeviceToHost));
    if (args->vtarget_out) HIP_TRY(hipMemcpy(args->vtarget_out, a.vtarget, U * T * sizeof(float), hipMemcpyDeviceToHost));
    if (args->loss_trace_out) HIP_TRY(hipMemcpy(args->loss_trace_out, a.trace, trace_n * sizeof(float), hipMemcpyDeviceToHost));
    if (hc && hc->factor_out) HIP_TRY(hipMemcpy(hc->factor_out, x.factor, U * T * sizeof(float), hipMemcpyDeviceToHost));
    // Buffer_for_PPO.clear() (MAPPO.py:481-482, IPPO.py:321-322, HAPPO.py:456-458): counters only
    for (int p = 0; p < h.P; ++p) { e->index[p] = 0; e->size[p] = 0; }
    return FRL_OK;
}

extern "C" int frl_mappo_learn(frl_engine* e, const frl_mappo_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    if (!is_mappo(e->h.algo)) return wrong_engine(e->h, "frl_mappo_learn");
    return mappo_learn_chain(e, args, nullptr);
}
