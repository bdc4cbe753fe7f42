"""The eight-wave chained actor stage (kernels_actor2.hip) parks pass A's second hidden layer h2 in lane-private slots of global
memory (csrc/actor_park_layout.h) and pass C loads it back instead of running the actor's forward a second time (the first layer is
formed again, the head's tanh is pass A's action).  Passes A and C call the same forward on the same rows in the same row-to-lane
mapping, so the parked registers ARE what pass C used to recompute: the update must not change by a bit.

FRL_ACTOR_PARK (read once, at create) picks the kernel: 1 = parked (the default), 0 = the recompute kernel; Engine.actor_park()
reports the kernel that was resolved, and every engine of a pair is asserted to run the one its knob names.  Every case builds one
engine of each kind, with FRL_CRITIC_V2=1 so that one and three learners take the chained kernels (learn_path()[0] is asserted), the
same seed, the same per-learner parameters and the same ring — only as large as the draw needs, 2 x batch rows — and makes four
learn() calls with device-drawn rows.  Compared by np.array_equal, for every learner: online and target parameters, Adam m and v of
both nets, the step counts, SAC's alpha state, and the stats of every call.

    algorithm   TD3 (do_actor on calls 1 and 3: the policy step is delayed), DDPG, SAC
    learners    1 and 3 (a wrong learner stride of the park buffer shows from two learners up)
    batch       1 (one lane), 16 / 17 (a full tile and one row more), 128 / 129 (one chunk and one row more), 255 (a ragged last tile),
                256 (the full carve)
    obs / act   8 / 2, 3 / 1, 12 / 4

The four-wave kernel (FRL_CHAIN_WAVES=4) maps pass A's rows differently and stays on the recompute path: the knob must change nothing
there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CALLS = 4
KW = dict(gamma=0.99, tau=0.005, actor_lr=1e-3, critic_lr=1e-3)
ALGOS = ["TD3", "DDPG", "SAC"]
LEARNERS = [1, 3]
BATCHES = [1, 16, 17, 128, 129, 255, 256]
SHAPES = [(8, 2), (3, 1), (12, 4)]


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


def _run(N, monkeypatch, algo, P, B, O, A, park, waves=None):
    """Four learn() calls on an engine created under FRL_ACTOR_PARK=park -> every array the update writes, and the stats per call"""
    from freerl_amd.engine import Engine
    monkeypatch.setenv("FRL_CRITIC_V2", "1")
    monkeypatch.delenv("FRL_SOLO", raising=False)
    monkeypatch.setenv("FRL_ACTOR_PARK", park)
    if waves:
        monkeypatch.setenv("FRL_CHAIN_WAVES", waves)
    else:
        monkeypatch.delenv("FRL_CHAIN_WAVES", raising=False)
    cap = 2 * B
    e = Engine(getattr(N, "ALGO_" + algo), O, A, cap, n_learners=P, twin_critic=(algo != "DDPG"), batch_max=B, seed=7)
    assert e.learn_path(B)[0], "%s (%d, %d) batch %d did not take the register-chained kernels: %r" % (algo, O, A, B, e.learn_path(B))
    # the kernel frl_create resolved, not the knob: the two engines of a pair must differ here, or the comparison is of a kernel with itself
    assert e.actor_park() == (park == "1" and not waves), "FRL_ACTOR_PARK=%s waves %s: actor_park() says %r" % (park, waves, e.actor_park())
    rng = np.random.default_rng(1000 * O + A)
    for net in range(2):
        for p in range(P):          # distinct per learner, online = target
            flat = (rng.standard_normal(e.num_params(net)) * 0.1).astype(np.float32)
            e.set_params(net, flat, N.PARAM_ONLINE, learner=p)
            e.set_params(net, flat, N.PARAM_TARGET, learner=p)
    e.fill_synthetic(cap, seed=5)
    stats = []
    for k in range(CALLS):
        if algo == "SAC":
            st = e.learn(B, alpha_lr=1e-4, target_entropy=-float(A), want_stats=True, **KW)
        elif algo == "DDPG":
            st = e.learn(B, want_stats=True, **KW)
        else:
            st = e.learn(B, do_actor=(k % 2 == 1), use_policy_noise=True, policy_noise=0.2, noise_clip=0.5, max_action=1.0, want_stats=True, **KW)
        assert np.all(np.isfinite(st))
        stats.append(st)
    out = {}
    for p in range(P):
        for net in range(2):
            for kind, name in ((N.PARAM_ONLINE, "online"), (N.PARAM_TARGET, "target"), (N.PARAM_ADAM_M, "m"), (N.PARAM_ADAM_V, "v")):
                out["learner %d net %d %s" % (p, net, name)] = e.get_params(net, kind, learner=p)
            out["learner %d net %d step" % (p, net)] = np.array(e.opt_step(net, learner=p))
        if algo == "SAC":
            v, t = e.alpha_state(learner=p)
            out["learner %d alpha" % p] = np.append(v, np.float32(t))
    out["stats"] = np.stack(stats)
    e.close()
    return out


def _assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s differs between FRL_ACTOR_PARK=0 and 1" % k


@pytest.mark.parametrize("O,A", SHAPES, ids=["o%d-a%d" % s for s in SHAPES])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("P", LEARNERS)
@pytest.mark.parametrize("algo", ALGOS)
def test_parked_activations_change_no_bit(N, monkeypatch, algo, P, B, O, A):
    recompute = _run(N, monkeypatch, algo, P, B, O, A, "0")
    parked = _run(N, monkeypatch, algo, P, B, O, A, "1")
    # the policy step did run (TD3: on two of the four calls), or the comparison would be of two untouched actors
    assert int(parked["learner 0 net 0 step"]) == (CALLS // 2 if algo == "TD3" else CALLS)
    _assert_same_bits(recompute, parked)


def test_four_wave_kernel_ignores_the_knob(N, monkeypatch):
    recompute = _run(N, monkeypatch, "TD3", 3, 129, 8, 2, "0", waves="4")
    parked = _run(N, monkeypatch, "TD3", 3, 129, 8, 2, "1", waves="4")
    _assert_same_bits(recompute, parked)
