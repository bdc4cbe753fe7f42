// frl_envelope_ddpg_learn (include/freerl_hip.h): ENVELOPE_DDPG.learn (ENVELOPE_MORL_file/ENVELOPE_DDPG.py:254-320) for a population.
// Included by frl_api.hip.
//
// Launch chain: envelope_prelude (frl_api_envelope.inc: [draw_kernel] -> envelope_weights_kernel) -> envelope_ddpg_critic_kernel ->
// reduce + clip 0.5 + Adam of the critic (net 1) -> envelope_ddpg_actor_kernel (through the critic just stepped) -> reduce + clip 0.5
// + Adam of the actor (net 0).  Each Adam launch carries its net's soft update, as the DDPG launcher folds it: the reference moves
// both targets after both steps (:308-320), but the actor step reads the ONLINE critic only and leaves it alone, and nothing reads
// actor_target, so the targets end where the reference's do.

extern "C" int frl_envelope_ddpg_learn(frl_engine* e, const frl_envelope_ddpg_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    const EngineDesc& h = e->h;
    if (h.algo != ALGO_ENVELOPE_DDPG) return wrong_engine(h, "frl_envelope_ddpg_learn");
    EnvelopeLaunch L;
    if (const int rc = envelope_prelude(e, {args->batch, args->weight_num, args->gamma, args->beta, args->idx, args->weights},
                                        {args->gamma, args->tau, args->actor_lr, args->critic_lr, args->beta},
                                        "gamma / tau / actor_lr / critic_lr / beta", &L)) return rc;
    AdamArgs ad{};
    ad.batch = L.rows;                             // the loss partials are per row
    ad.eps = 1e-8f; ad.beta1 = 0.9f; ad.beta2 = 0.999f;
    ad.clip = 0.5f; ad.soft = 1; ad.tau = args->tau;
    ad.which = 0; ad.lr = args->critic_lr;         // net 1: beta d^2 + (1 - beta) / R sum_k e_k^2 per row
    launch_rowchunk_update(e, e->stream, h.P, 0, L.ns, ad, envelope_ddpg_critic_kernel, L.a);
    ad.which = 1; ad.lr = args->actor_lr;          // net 0: -sum_k Q_k / R per row
    launch_rowchunk_update(e, e->stream, h.P, 0, L.ns, ad, envelope_ddpg_actor_kernel, L.a);
    HIP_TRY(hipGetLastError());
    if (!args->critic_loss_out && !args->actor_loss_out && !args->weights_out) return FRL_OK;
    return read_back(e, args->weights_out, args->weight_num, {ST_CRITIC_LOSS, args->critic_loss_out}, {ST_ACTOR_LOSS, args->actor_loss_out});
}
