#!/usr/bin/env python
"""Record tests/golden/ref_runs.npz: what the reference's OWN code answered on the cases of tests/test_ref_vecenv.py
(the lock-step executor over NormalizedEnv, oracle/ref_vecenv.py) and tests/test_sampler_contract_host.py (the
VectorizedSampler loop on a replayed recording, oracle/ref_vecsampler.py) -- outputs only, next to the case names
(TEST INFRASTRUCTURE; needs the staged reference, so it runs where `python oracle/make_ref.py` can).  The tests hold
the oracle to these recordings wherever the reference is not staged, and require a live run to reproduce them where
it is.

    python oracle/make_golden_refruns.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TESTS = os.path.join(ROOT, "tests")
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_ref_vecenv as V
    import test_sampler_contract_host as S
    assert V.HAVE_REF, "no staged reference: run `python oracle/make_ref.py` first"
    out = {}

    def put(case, rec):
        for k, v in rec.items():
            out["%s/%s" % (case, k)] = np.array(json.dumps(v, sort_keys=True)) if k == "modules" else np.asarray(v)

    for kind, mpl in V.LOCK_STEP_CASES:
        draws, actions = V.lock_step_inputs(kind)
        put("lock_step_k%d_m%d" % (kind, mpl), V.lock_step_reference(kind, mpl, draws, actions))
    for want, whole, _, _ in S.LOOP_CASES:
        put(S.loop_case_name(want, whole), S.loop_reference(want, whole))
    try:
        S.loop_reference(12, True)
        raise AssertionError("the reference loop accepted a recording that is too short")
    except RuntimeError as err:
        msg = [l for l in str(err).splitlines() if "asks for lock step" in l]
        put("vec_sampler_loop_too_short", {"error": msg[-1].strip() if msg else str(err), "modules": {}})
    path = os.path.join(TESTS, "golden", "ref_runs.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
