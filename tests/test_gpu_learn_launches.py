"""Which launches one frl_learn() call makes, per kernel family: the per-slot launch counts of the engine's profile (times ignored)
and learn_path() next to them.  The host picks the family, skips the draw where a critic launch draws for itself (kernels_solo.hip,
single-agent kernels_solow.hip, the one-launch DQN update) or where the previous launch's spare workgroups already did (multi-agent
kernels_solow.hip), folds a policy step into one launch (kernels_solow.hip with helpers) and leaves reduce + Adam and MADDPG's soft
update to the chained kernels: every one of those decisions shows in the counts.  Shapes are the smallest that select the family."""
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("FRL_CRITIC_V2", "FRL_SOLO", "FRL_SOLOW", "FRL_DQN_FUSED", "FRL_SOLOW_FUSE", "FRL_SOLO_PREDRAW")
SLOTS = ("draw", "grad_critic", "adam_critic", "grad_actor", "adam_actor", "soft_update")
# dynamic LDS of the chained families' launches (kernels.h / frl_desc.h: critic8_lds_floats, solo_lds_floats, solow_lds_floats,
# wide_lds_floats, wide16_lds_floats_host, dqn2_lds_floats)
CHAIN8_LDS = 4 * (8 * 256 + 64 * 256 + 8 * 256 + 2 * 8192 + 128 + 128 + 16 + 16 + 256 * 4 + 3 * 256 + 64 + 1024)
SOLO_LDS = 117376
SOLOW_LDS = 4 * (64 * 256 + 2 * 8 * 256 + 128 + 128 + 32 + 32 + 4 * 8 * 256 + 26 * 256 + 3 * 256 + 256 + 4 * 2 * 256 + 16 * 32 + 16 * 48 + 128)
WIDE_LDS = 4 * (8 * 8 * 256 + 2 * 8 * 256 + 2 * 8192 + 128 + 128 + 32 + 32 + 64)
WIDE16_LDS = 4 * (16384 + 2 * 16 * 256 + 3 * 16 * 256 + 256 + 256 + 32 + 32 + 192)
DQN2_LDS = 77184
ROWCHUNK = "row-chunk"          # learn_path: (False, the engine's lds_bytes(), its row chunk)

MA_OBS, MA_ACT = [6, 5, 7], [2, 3, 2]
TD3_KW = dict(use_policy_noise=True, policy_noise=0.2, noise_clip=0.5, max_action=1.0)
SAC_KW = dict(alpha_lr=1e-4, target_entropy=-3.0)

# (id, engine, env, learn kwargs, calls, counts in SLOTS order summed over the calls, learn_path)
CASES = [
    ("td3_rowchunk", dict(algo="TD3", obs=8, act=2, P=2, B=64, twin=True), {"FRL_CRITIC_V2": "0"}, dict(do_actor=True, **TD3_KW), 1, (1, 1, 1, 1, 1, 0), ROWCHUNK),
    ("td3_rowchunk_critic_only", dict(algo="TD3", obs=8, act=2, P=2, B=64, twin=True), {"FRL_CRITIC_V2": "0"}, dict(do_actor=False, **TD3_KW), 1, (1, 1, 1, 0, 0, 0), ROWCHUNK),
    ("maddpg_rowchunk", dict(algo="MADDPG", obs=MA_OBS, act=MA_ACT, P=1, B=64), {"FRL_CRITIC_V2": "0"}, dict(do_actor=True), 1, (1, 1, 1, 1, 1, 1), ROWCHUNK),
    ("dqn_fused", dict(algo="DQN", obs=4, act=2, P=1, B=64, discrete=True), {}, {}, 1, (0, 1, 0, 0, 0, 0), (True, DQN2_LDS, 64)),
    ("dqn_rowchunk", dict(algo="DQN", obs=4, act=2, P=1, B=64, discrete=True), {"FRL_DQN_FUSED": "0"}, {}, 1, (1, 1, 1, 0, 0, 0), ROWCHUNK),
    ("td3_chained", dict(algo="TD3", obs=8, act=2, P=2, B=100, twin=True), {"FRL_CRITIC_V2": "1"}, dict(do_actor=True, **TD3_KW), 1, (1, 1, 0, 1, 0, 0), (True, CHAIN8_LDS, 100)),
    ("td3_solo", dict(algo="TD3", obs=8, act=2, P=1, B=100, twin=True), {}, dict(do_actor=True, **TD3_KW), 1, (0, 1, 0, 1, 0, 0), (True, SOLO_LDS, 16)),
    ("sac_solow_fused_step", dict(algo="SAC", obs=40, act=3, P=1, B=64, twin=True), {}, SAC_KW, 1, (0, 1, 0, 0, 0, 0), (True, SOLOW_LDS, 16)),
    ("sac_solow_two_launches", dict(algo="SAC", obs=40, act=3, P=1, B=64, twin=True), {"FRL_SOLOW_FUSE": "0"}, SAC_KW, 1, (0, 1, 0, 1, 0, 0), (True, SOLOW_LDS, 16)),
    # the one place where the HOST decides whether draw_kernel runs: the first call draws, the second takes the rows the first critic launch's spare workgroups drew
    ("maddpg_solow_predrawn", dict(algo="MADDPG", obs=MA_OBS, act=MA_ACT, P=1, B=64), {}, dict(do_actor=True), 2, (1, 2, 0, 2, 0, 0), (True, SOLOW_LDS, 16)),
    ("matd3_solow", dict(algo="MADDPG", obs=MA_OBS, act=MA_ACT, P=1, B=64, twin=True), {}, dict(do_actor=True, **TD3_KW), 2, (2, 2, 0, 2, 0, 0), (True, SOLOW_LDS, 16)),
    ("sac_wide", dict(algo="SAC", obs=40, act=3, P=2, B=64, twin=True), {"FRL_CRITIC_V2": "1"}, SAC_KW, 1, (1, 1, 0, 1, 0, 0), (True, WIDE_LDS, 64)),
    ("maddpg_wide", dict(algo="MADDPG", obs=MA_OBS, act=MA_ACT, P=2, B=64), {"FRL_CRITIC_V2": "1"}, dict(do_actor=True), 1, (1, 1, 0, 1, 0, 1), (True, WIDE_LDS, 64)),
    ("td3_h256_x_stationary", dict(algo="TD3", obs=8, act=2, P=2, B=64, twin=True, hidden=256), {"FRL_CRITIC_V2": "1"}, dict(do_actor=True, **TD3_KW), 1, (1, 1, 0, 1, 0, 0),
     (True, WIDE16_LDS, 64)),
]


@pytest.mark.parametrize("eng,env,kw,calls,counts,path", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_launches_of_a_learn_call(monkeypatch, eng, env, kw, calls, counts, path):
    from freerl_amd import _native as N
    from freerl_amd.engine import Engine
    assert N.device_count() > 0
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = eng["B"]
    e = Engine(getattr(N, "ALGO_" + eng["algo"]), eng["obs"], eng["act"], 1024, n_learners=eng["P"], twin_critic=eng.get("twin", False),
               batch_max=B, hidden=eng.get("hidden", 128), discrete=eng.get("discrete", False), seed=7)
    try:
        e.fill_synthetic(400, seed=3)
        e.profile(True)
        for _ in range(calls):
            e.learn(B, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, **kw)          # device-drawn rows (and noise)
        prof = e.profile_read()
        got = tuple(int(prof.get(s, (0.0, 0))[1]) for s in SLOTS)
        want_path = (False,) + e.lds_bytes() if path == ROWCHUNK else path
        got_path = e.learn_path(B)
        print("launches", dict(zip(SLOTS, got)), "learn_path", got_path)
        assert got == counts, dict(zip(SLOTS, got))
        assert set(prof) <= set(SLOTS), prof
        assert got_path == want_path
    finally:
        e.close()
