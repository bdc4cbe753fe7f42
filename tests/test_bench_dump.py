"""bench.py --dump-outputs on CPU: the files dump_outputs writes for a stand-in engine of the bench's shape (names, dtype,
shapes, the fixed learner sample, the 64 MB bound).  The GPU run of the same path is bench.py itself."""
import glob
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _FakeEngine:
    """get_params of a bench-shaped TD3 population (hidden 128, obs 8, act 2, twin critic): learner p's values encode
    (p, net, kind), so a test can tell which learner a row came from."""
    SIZES = {0: 128 * 8 + 128 + 128 * 128 + 128 + 2 * 128 + 2, 1: 2 * (128 * 10 + 128 + 128 * 128 + 128 + 128 + 1)}

    def __init__(self, P):
        self.P = P

    def get_params(self, net, kind=0, learner=0):
        return np.full(self.SIZES[net], learner * 100 + net * 10 + kind, dtype=np.float32)


def _dump(tmp_path, P):
    from freerl_amd import _native as N
    b = _bench()
    stats = np.arange(P * N.FRL_STAT_COUNT, dtype=np.float32).reshape(P, 1, N.FRL_STAT_COUNT)
    out = tmp_path / ("P%d" % P)
    b.dump_outputs(N, _FakeEngine(P), stats, str(out))
    return b, N, stats, {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(out / "*.npy"))}


def test_dump_outputs_population(tmp_path):
    b, N, stats, got = _dump(tmp_path, 512)
    assert sorted(got) == ["actor_online", "actor_target", "critic_online", "critic_target", "stats"]
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["stats"], stats)
    total = sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "P512" / "*.npy")))
    assert total <= 64 * 2 ** 20, total
    rows = got["critic_online"][:, 0] // 100
    assert got["critic_online"].shape == (b.DUMP_LEARNERS, _FakeEngine.SIZES[1])
    assert len(set(rows)) == b.DUMP_LEARNERS and np.all(np.diff(rows) > 0) and rows.max() < 512
    for name, net, kind in (("actor_online", 0, N.PARAM_ONLINE), ("actor_target", 0, N.PARAM_TARGET),
                            ("critic_online", 1, N.PARAM_ONLINE), ("critic_target", 1, N.PARAM_TARGET)):
        np.testing.assert_array_equal(got[name][:, 0], rows * 100 + net * 10 + kind)
    # the sample is fixed: a second dump picks the same learners
    assert np.array_equal(_dump(tmp_path / "again", 512)[3]["critic_online"][:, 0] // 100, rows)


def test_dump_outputs_small_population_writes_every_learner(tmp_path):
    _, _, _, got = _dump(tmp_path, 3)
    np.testing.assert_array_equal(got["actor_online"][:, 0] // 100, [0, 1, 2])
