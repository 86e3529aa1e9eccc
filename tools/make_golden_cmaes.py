#!/usr/bin/env python
"""Replay fixtures of CMAState: the reference's own CMA-ES library, run and recorded.

Loads rllab/algos/cma_es_lib.py of a reference checkout IN MEMORY (nothing of its text is written anywhere), runs
``CMAEvolutionStrategy(x0, sigma0, options)`` on a noisy quadratic and writes, per case, tests/golden/cmaes_ref_<case>.npz:
x0, sigma0, the options, every iteration's told ``xs`` / ``fs``, after every ``tell`` the mean, sigma, pc, ps, dC, the sorted
D, count_eigen and the keys of ``stop()``, C at a few iterations and at the end, ``result()[0]``, and the strategy constants.
tests/golden/cmaes_ref_constants.npz holds the constants alone for N = 2, 24, 1250.

The library is from 2015; on a current Python / NumPy it needs exactly these changes, applied to the text in memory:
``collections.MutableMapping`` -> ``collections.abc.MutableMapping``, ``time.clock()`` -> ``time.perf_counter()``,
``array(..., copy=False)`` -> ``copy=None`` (what it meant before NumPy 2), ``np.NaN`` / ``np.Inf`` defined in-process; x0 is
passed as a list and the options ``verbose=-9, verb_log=0, verb_disp=0`` keep it from writing files.

Cases (N = 24, default popsize 13):
  plain        defaults, 12 iterations: one eigendecomposition per ask from iteration 1 (the plain negative update)
  wait3        updatecovwait=3, 20 iterations: every fourth ask does 3 (the two-extra-eigendecompositions branch, unclipped)
  wait8_ask40  updatecovwait=8, 30 iterations, ask(40) and tell a PREFIX of 20..28 of them (the batch_size path of
               rllab/algos/cma_es.py:98-117: more told than popsize, fewer than asked): 3 eigendecompositions per update.
               Telling all 40 would make the file 230 kB of incompressible float64 points, above the largest fixture of
               tests/golden (203 kB); the prefix keeps it below.
  inactive     CMA_active=False, 12 iterations

  python tools/make_golden_cmaes.py [--reference /path/to/rllab] [--out tests/golden] [--case NAME]
"""
import argparse
import collections
import collections.abc
import os
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_REFERENCE = "/root/reference"
LIB_OPTS = {"verbose": -9, "verb_log": 0, "verb_disp": 0}

CASES = collections.OrderedDict([
    ("plain", dict(N=24, opts={}, n_itr=12, ask=None, seed=11)),
    ("wait3", dict(N=24, opts={"updatecovwait": 3}, n_itr=20, ask=None, seed=12)),
    ("wait8_ask40", dict(N=24, opts={"updatecovwait": 8}, n_itr=30, ask=40, seed=13)),
    ("inactive", dict(N=24, opts={"CMA_active": False}, n_itr=12, ask=None, seed=14)),
])
C_EVERY = {"plain": 5, "wait3": 5, "wait8_ask40": 10, "inactive": 5}
CONSTANT_NS = (2, 24, 1250)


def load_library(reference=DEFAULT_REFERENCE):
    """The library as a module object, compiled from its patched text."""
    path = os.path.join(reference, "rllab", "algos", "cma_es_lib.py")
    text = open(path).read()
    n_before = len(text)
    text = text.replace("collections.MutableMapping", "collections.abc.MutableMapping")
    text = text.replace("time.clock()", "time.perf_counter()")
    # NumPy 2 reads copy=False as "never copy" and raises where NumPy 1 copied when it had to; copy=None is the old meaning
    text = text.replace(", copy=False)", ", copy=None)")
    assert len(text) != n_before
    if not hasattr(np, "NaN"):
        np.NaN = np.nan
    if not hasattr(np, "Inf"):
        np.Inf = np.inf
    mod = types.ModuleType("cma_es_lib_in_memory")
    mod.__file__ = path
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SyntaxWarning)        # `x is 1` comparisons of its time
        exec(compile(text, path, "exec"), mod.__dict__)
    return mod


def told_count(case, itr, asked):
    """How many of the asked points are told: all, or (wait8_ask40) a prefix of 20..28 as a batch_size cut would leave."""
    return asked if CASES[case]["ask"] is None else 20 + (itr * 5) % 9


def fitness(x, rng, target, scale):
    """A noisy quadratic with continuous values: sum_i scale_i (x_i - target_i)^2 times (1 + 0.1 N(0, 1))."""
    return float(np.sum(scale * (x - target) ** 2) * (1.0 + 0.1 * rng.randn()))


def constants(es):
    sp = es.sp
    es.adapt_sigma.initialize(es)
    neg = sp.neg
    return dict(popsize=sp.popsize, mu=sp.mu, lam_mirr=sp.lam_mirr, mueff=sp.mueff, cc=sp.cc, c1=sp.c1, cmu=sp.cmu,
                cmean=sp.cmean, weights=np.array(sp.weights), cs=es.adapt_sigma.cs, damps=es.adapt_sigma.damps,
                chiN=es.const.chiN, neg_mu=getattr(neg, "mu", 0), neg_weights=np.array(getattr(neg, "weights", np.zeros(0))),
                neg_mueff=getattr(neg, "mueff", 0.0), neg_cmuexp=neg.cmuexp, maxiter=es.opts["maxiter"],
                tolstagnation=es.opts["tolstagnation"])


def run_case(lib, name):
    spec = CASES[name]
    N, seed = spec["N"], spec["seed"]
    rng = np.random.RandomState(seed)
    x0 = rng.randn(N)
    sigma0 = 0.5
    target = rng.randn(N)
    scale = np.exp(rng.uniform(-1.0, 1.0, N))
    opts = dict(LIB_OPTS, seed=seed, **spec["opts"])
    es = lib.CMAEvolutionStrategy(list(x0), sigma0, opts)
    out = dict(x0=x0, sigma0=np.float64(sigma0), n_itr=np.int64(spec["n_itr"]),
               option_names=np.array(sorted(spec["opts"])), option_values=np.array([float(spec["opts"][k]) for k in sorted(spec["opts"])]))
    for k, v in constants(es).items():
        out["const_" + k] = np.asarray(v, dtype=np.float64)
    eig_per_ask, rec = [], collections.defaultdict(list)
    for itr in range(spec["n_itr"]):
        before = es.count_eigen
        xs = np.asarray(es.ask() if spec["ask"] is None else es.ask(spec["ask"]))
        eig_per_ask.append(es.count_eigen - before)
        xs = xs[:told_count(name, itr, len(xs))]
        fs = np.array([fitness(x, rng, target, scale) for x in xs])
        assert len(set(fs.tolist())) == len(fs), "ties in fs"
        es.tell(xs, fs)
        stop = es.stop()
        for k, v in (("xs", xs), ("fs", fs), ("lam", len(fs)), ("mean", es.mean), ("sigma", es.sigma), ("pc", es.pc),
                     ("ps", es.adapt_sigma.ps), ("dC", es.dC), ("D", np.sort(np.array(es.D))), ("count_eigen", es.count_eigen),
                     ("stop", "|".join(sorted(stop.keys())))):
            rec[k].append(np.array(v))
        if (itr + 1) % C_EVERY[name] == 0 or itr == spec["n_itr"] - 1:
            rec["C_iters"].append(itr)
            rec["C"].append(np.array(es.C))
    # one array per quantity, iterations along axis 0 (xs / fs: the iterations' rows one after the other, ``lam`` each)
    for k, v in rec.items():
        out[k] = np.concatenate(v) if k in ("xs", "fs") else np.stack(v)
    out["eig_per_ask"] = np.array(eig_per_ask, dtype=np.int64)
    out["result_x"] = np.array(es.result()[0])
    out["result_f"] = np.float64(es.result()[1])
    # the branches each case is there for
    e = eig_per_ask
    if name in ("plain", "inactive"):
        assert e[0] == 0 and all(v == 1 for v in e[1:]), e
    elif name == "wait3":
        assert [v for v in e if v] == [3] * (len([v for v in e if v])) and e[4::4] == [3] * len(e[4::4]) and sum(e) == 3 * len(e[4::4]), e
    elif name == "wait8_ask40":
        assert [v for v in e if v] == [3] * len([v for v in e if v]) and len([v for v in e if v]) >= 3, e
        assert all(l > es.sp.popsize for l in out["lam"])
    return out


def run_constants(lib):
    out = {}
    for N in CONSTANT_NS:
        es = lib.CMAEvolutionStrategy([0.0] * N, 1.0, dict(LIB_OPTS, seed=1))
        for k, v in constants(es).items():
            out["N%d_%s" % (N, k)] = np.asarray(v, dtype=np.float64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=DEFAULT_REFERENCE)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    lib = load_library(args.reference)
    limit = max(os.path.getsize(os.path.join(args.out, f)) for f in os.listdir(args.out) if not f.startswith("cmaes_ref_"))
    jobs = [(n, lambda n=n: run_case(lib, n)) for n in CASES if args.case in (None, n)]
    if args.case in (None, "constants"):
        jobs.append(("constants", lambda: run_constants(lib)))
    for name, job in jobs:
        path = os.path.join(args.out, "cmaes_ref_%s.npz" % name)
        np.savez_compressed(path, **job())
        size = os.path.getsize(path)
        print("%s: %d bytes (limit %d)" % (path, size, limit))
        assert size <= limit, "fixture larger than the largest file already under tests/golden"


if __name__ == "__main__":
    main()
