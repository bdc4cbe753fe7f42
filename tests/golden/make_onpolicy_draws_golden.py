#!/usr/bin/env python3
"""tests/golden/onpolicy_draws.npz: what one `perms=None` learn call of each on-policy entry point leaves in the nets, recorded from
the library as built from the commit BEFORE the on-policy call plan (csrc/onpolicy_plan.hpp) — the draws a call takes, and the order
it takes them in, are part of the library's behaviour, and this file is what holds them.  Run by hand on a machine with a HIP device:

    python -m tests.golden.make_onpolicy_draws_golden [OUT.npz]

Re-record only for a change that is meant to move the draws.  Per case (tests/onpolicy_draws_cases.py) the maker also runs a second
engine with another seed and refuses to write a fixture in which that one ends with the same bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import onpolicy_draws_cases as oc  # noqa: E402


def main(out_path):
    from freerl_amd import _native as N
    assert N.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    out = {}
    for entry, T, mb in oc.CASES:
        key = oc.name(entry, T, mb)
        a, again, other = oc.run(N, entry, T, mb), oc.run(N, entry, T, mb), oc.run(N, entry, T, mb, seed=oc.OTHER_SEED)
        assert np.array_equal(a, again), key + ": two engines of one seed differ"
        n_diff = int(np.count_nonzero(a != other))
        print("%s: %d floats, %d differ under seed %d" % (key, a.size, n_diff, oc.OTHER_SEED), flush=True)
        assert n_diff > 0, key + ": the seed does not reach the result"
        out[key] = a
    np.savez(out_path, **out)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "onpolicy_draws.npz"))
