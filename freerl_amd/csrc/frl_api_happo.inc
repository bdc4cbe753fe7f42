// HAPPO entry point (included at the end of frl_api.hip, behind frl_api_mappo.inc).

extern "C" int frl_happo_learn(frl_engine* e, const frl_happo_args* args) {
    ENG(e);
    if (!args) return fail(FRL_ERR_INVALID, "args is NULL");
    if (e->h.algo != ALGO_HAPPO) return wrong_engine(e->h, "frl_happo_learn");
    // frl_happo_args is frl_mappo_args' fields, in order, and two more behind them
    static_assert(offsetof(frl_happo_args, agent_order) == sizeof(frl_mappo_args), "frl_happo_args begins with frl_mappo_args' fields");
    frl_mappo_args m;
    memcpy(&m, args, sizeof m);
    const HappoCall hc = {args->agent_order, args->factor_out};
    return mappo_learn_chain(e, &m, &hc);
}
