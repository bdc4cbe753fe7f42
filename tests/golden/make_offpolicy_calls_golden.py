#!/usr/bin/env python3
"""tests/golden/offpolicy_calls.npz: the rows three consecutive device-drawn calls of every off-policy entry point train on, what the
calls return and a digest of every net afterwards, recorded from the library as built from the commit BEFORE the off-policy call plan
(csrc/learn_plan.hpp) — the draws a call takes, the order it takes them in and the launches it makes are part of the library's
behaviour, and this file is what holds them.  Run by hand on a machine with a HIP device:

    python -m tests.golden.make_offpolicy_calls_golden [OUT.npz]

Re-record only for a change that is meant to move the draws.  Per case (tests/offpolicy_calls_cases.py) the maker runs a second engine of
the same seed: the rows must be the same bits (or the case is dropped), and a case whose outputs or digest are not keeps its rows only;
either is named in the fixture's `notes`, and more than two of them refuse the fixture.  A third engine with another seed must draw
other rows."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import offpolicy_calls_cases as oc  # noqa: E402


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main(out_path):
    from freerl_amd import _native as N
    assert N.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    out, notes = {}, []
    for name in oc.NAMES:
        a, again, other = oc.run(N, name), oc.run(N, name), oc.run(N, name, seed=oc.OTHER_SEED)
        keep = sorted(a)
        if "idx" in a:
            if not _same(a["idx"], again["idx"]):
                notes.append(name + ": dropped, two engines of one seed drew different rows")
                continue
            assert not _same(a["idx"], other["idx"]), name + ": the seed does not reach the draws"
        if not (_same(a["out"], again["out"]) and _same(a["digest"], again["digest"])):
            notes.append(name + ": rows only, outputs or parameters differ between two engines of one seed")
            keep = ["idx"]
        print("%s: keeps %s" % (name, ", ".join("%s%s" % (k, a[k].shape) for k in keep)), flush=True)
        for k in keep:
            out[name + "/" + k] = a[k]
    assert len(notes) <= 2, notes
    out["notes"] = np.array("; ".join(notes))
    np.savez_compressed(out_path, **out)
    print("notes: %s" % (notes or "none"))
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "offpolicy_calls.npz"))
