import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def unpack_paths(g):
    """Rebuild the list of path dicts stored by oracle/make_golden.py::pack."""
    paths, o = [], 0
    for L in g["lens"]:
        L = int(L)
        paths.append(dict(observations=g["observations"][o:o + L].copy(), actions=g["actions"][o:o + L].copy(),
                          rewards=g["rewards"][o:o + L].copy(),
                          agent_infos=dict(mean=g["mean"][o:o + L].copy(), log_std=g["log_std"][o:o + L].copy()),
                          env_infos=dict()))
        o += L
    return paths


STAT_KEYS = ['AverageDiscountedReturn', 'AverageReturn', 'ExplainedVariance', 'NumTrajs', 'Entropy',
             'Perplexity', 'StdReturn', 'MaxReturn', 'MinReturn']


REF_RUNS = "ref_runs"      # oracle/make_golden_refruns.py: the reference's own executor / sampler loop, recorded


def ref_run(case, live=None):
    """The reference's output for one recorded case of tests/golden/ref_runs.npz (arrays by name, ``modules`` as the
    dict the child reported).  ``live``, where the reference is staged: run it now as well and require the recording."""
    import json
    g = load(REF_RUNS)
    prefix = case + "/"
    rec = {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    assert rec, "no recorded reference run %r: regenerate with `python oracle/make_golden_refruns.py`" % case
    rec["modules"] = json.loads(str(rec["modules"]))
    if live is not None:
        out = live()
        assert set(out) == set(rec), (case, sorted(set(out) ^ set(rec)))
        for k, v in rec.items():
            assert (out[k] == v) if k == "modules" else np.array_equal(np.asarray(out[k]), v), (case, k)
    return rec
