"""The two CPU figures behind tests/test_gpu_beta_act.py (DESIGN.md "Beta draw"); needs no GPU.
    python tools/beta_act_gap.py
1. The float32 gap of the Beta log-density on test_logp_and_range's inputs: the float64 density on the float64 head rows z of a float64
   forward against the same density on z rounded to float32, at SciPy's draws x (rounded to float32 and clamped as the kernel clamps).
   The test's bound is 4 x the largest.  Next to it, the kernel's arithmetic rehearsed in NumPy: float32 softplus, the rest in double,
   stored as float32.
2. The Kolmogorov-Smirnov distance of SciPy's own Beta sampler at the law test's n and shapes, over 20 seeds, against the DKW bound."""
import numpy as np
from scipy import stats
from scipy.special import betaln

O, H, N_LAW = 5, 128, 8192


def logpdf(s, x, A):                               # s = softplus(z) in float64
    al, be = s[:, :A] + 1, s[:, A:] + 1
    return (al - 1) * np.log(x) + (be - 1) * np.log1p(-x) - betaln(al, be)


def head_rows(obs, par, A):                        # float64 forward of the engine's net: [l1.w l1.b l2.w l2.b head.w head.b], ReLU trunk
    o, h = 0, obs.astype(np.float64)
    for n_out, n_in, relu in ((H, O, True), (H, H, True), (2 * A, H, False)):
        w, b = par[o:o + n_out * n_in].reshape(n_out, n_in), par[o + n_out * n_in:o + n_out * n_in + n_out]
        o += n_out * n_in + n_out
        h = h @ w.astype(np.float64).T + b
        h = np.maximum(h, 0) if relu else h
    return h


if __name__ == "__main__":
    gap = kern = 0.0
    for n_rows in (1, 17, 65):
        for A in (1, 3, 8, 17):
            g = np.random.default_rng(1000 * n_rows + A)                   # the test's own draws, in its order
            obs = g.standard_normal((2, n_rows, O)).astype(np.float32)
            par = (g.standard_normal((2, H * O + H + H * H + H + 2 * A * H + 2 * A)) * 0.1).astype(np.float32)
            par[:, -2 * A:] = g.standard_normal((2, 2 * A)) * 1.5
            for p in range(2):
                z64 = head_rows(obs[p], par[p], A)
                z32 = z64.astype(np.float32)
                sp = lambda z: np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20))))
                x = stats.beta(sp(z64[:, :A]) + 1, sp(z64[:, A:]) + 1).rvs(random_state=np.random.default_rng(7))
                x = np.clip(x.astype(np.float32), np.finfo(np.float32).tiny, np.float32(1 - 2.0 ** -24)).astype(np.float64)
                on32 = logpdf(sp(z32.astype(np.float64)), x, A)
                gap = max(gap, np.abs(logpdf(sp(z64), x, A) - on32).max())
                s32 = np.where(z32 > 20, z32, np.log1p(np.exp(z32), dtype=np.float32)).astype(np.float64)
                kern = max(kern, np.abs(logpdf(s32, x, A).astype(np.float32) - on32).max())
    print("log-density, float64 z against float32-rounded z: %.3e (4 x: %.3e); NumPy rehearsal of the kernel against float64: %.3e" % (gap, 4 * gap, kern))
    bound = np.sqrt(np.log(2 / 1e-6) / (2 * N_LAW))
    one = 1 + np.log1p(np.exp(-12.0))
    for al, be in ((one, one), (1.3, 9.0), (20.0, 20.0)):
        ks = max(stats.kstest(stats.beta(al, be).rvs(N_LAW, random_state=np.random.default_rng(s)), stats.beta(al, be).cdf).statistic for s in range(20))
        print("Beta(%.6g, %.6g): SciPy's sampler, n = %d, worst KS over 20 seeds %.4f (DKW bound at p = 1e-6: %.4f)" % (al, be, N_LAW, ks, bound))
