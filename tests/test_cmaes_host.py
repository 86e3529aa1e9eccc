"""CMA-ES on the host: CMAState against replays of the reference's own library (tests/golden/cmaes_ref_*.npz, written by
tools/make_golden_cmaes.py), its constants, the sampling identity, the clipped negative update, every stop criterion, the
constructor against rllab/algos/cma_es.py and the C ABI entry of the covariance update."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ["plain", "wait3", "wait8_ask40", "inactive"]

# Replay parity: the largest relative deviation (max-norm per quantity) from the fixtures, measured with
# replay_case: 3.14e-15 on the CPU, 3.36e-15 on the MI355X (both ps of wait8_ask40).
# The bound is 16 x the larger one -- room for the solver and the reduction order of another build -- and never above
# 1e-8: float64 state, at most 30 iterations, cond(C) < 2 in every case; anything above that is not rounding.
PARITY_MEASURED_CPU, PARITY_MEASURED_GPU = 3.14e-15, 3.36e-15
PARITY_TOL = 16 * max(PARITY_MEASURED_CPU, PARITY_MEASURED_GPU)
assert PARITY_TOL <= 1e-8


def fixture_options(g):
    opts = {}
    for k, v in zip(g["option_names"], g["option_values"]):
        k = str(k)
        opts[k] = bool(v) if k == "CMA_active" else int(v)
    return opts


def replay_case(case, device="cpu"):
    """Run CMAState through the recorded iterations of one fixture: ask (draws discarded), tell the recorded points.
    Returns (state, {quantity: largest relative deviation by max-norm}); count_eigen and the stop keys are asserted equal
    on the way.  B is not compared: every compared quantity is invariant to the choice of eigenbasis."""
    from rllab_amd.algos.cma_state import CMAState
    g = np.load(os.path.join(GOLDEN, "cmaes_ref_%s.npz" % case))
    es = CMAState(torch.as_tensor(g["x0"], device=device), float(g["sigma0"]), dict(fixture_options(g), seed=1))
    off, worst, c_iters = 0, {}, [int(i) for i in g["C_iters"]]

    def dev(name, got, ref):
        got = got.detach().cpu().numpy()
        worst[name] = max(worst.get(name, 0.0), float(np.abs(got - ref).max() / np.abs(ref).max()))
    for it in range(int(g["n_itr"])):
        lam = int(g["lam"][it])
        xs_asked = es.ask(None if case != "wait8_ask40" else 40)
        assert xs_asked.shape[0] == (40 if case == "wait8_ask40" else es.sp.popsize)
        es.tell(torch.as_tensor(g["xs"][off:off + lam], device=device), torch.as_tensor(g["fs"][off:off + lam], device=device))
        off += lam
        stop = es.stop()
        for name, got in (("mean", es.mean), ("sigma", es.sigma), ("pc", es.pc), ("ps", es.ps), ("dC", es.dC),
                          ("D", torch.sort(es.D).values)):
            dev(name, got, g[name][it])
        if it in c_iters:
            dev("C", es.C, g["C"][c_iters.index(it)])
        assert es.count_eigen == int(g["count_eigen"][it]), (case, it)
        assert "|".join(sorted(stop)) == str(g["stop"][it]), (case, it, stop)
    dev("result_x", es.result()[0], g["result_x"])
    assert abs(es.result()[1] - float(g["result_f"])) <= PARITY_TOL * abs(float(g["result_f"]))
    return es, worst


@pytest.mark.parametrize("case", CASES)
def test_replay_parity(case):
    es, worst = replay_case(case)
    print("replay %s (cpu): %s" % (case, {k: "%.2e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= PARITY_TOL, worst
    # the fixture is the branch it claims to be
    g = np.load(os.path.join(GOLDEN, "cmaes_ref_%s.npz" % case))
    e = [int(v) for v in g["eig_per_ask"]]
    if case in ("plain", "inactive"):
        assert e == [0] + [1] * (len(e) - 1)
    elif case == "wait3":
        assert e == [3 if (i and i % 4 == 0) else 0 for i in range(len(e))]
    else:
        assert set(e) == {0, 3} and e.count(3) >= 3 and int(g["lam"].min()) > es.sp.popsize


def _np_constants(N, popsize=None):
    """_CMAParameters.set / CMAAdaptSigmaCSA.initialize with the default options, restated in NumPy."""
    popsize = 4 + int(3 * np.log(N)) if popsize is None else popsize
    mu = max(int(0.5 * popsize + 0.499999), 1)
    w = np.log(max(mu, popsize / 2.0) + 0.5) - np.log(1 + np.arange(mu))
    w /= w.sum()
    mueff = 1 / (w ** 2).sum()
    wn = np.array([np.log(k) - np.log(popsize / 2 + 1 / 2) for k in np.arange(np.ceil(popsize / 2 + 1.1 / 2), popsize + .1)])
    wn /= wn.sum()
    neg_mueff = 1 / (wn ** 2).sum()
    cs = (mueff + 2) / (N + (mueff + 3))
    c1 = min(1, popsize / 6) * 2 / ((N + 1.3) ** 2 + mueff)
    return dict(popsize=popsize, mu=mu, neg_mu=len(wn), mueff=mueff, cs=cs, cc=(4 + mueff / N) / (N + (4 + 2 * mueff / N)), c1=c1,
                cmu=min(1 - c1, 2 * (0.3 + mueff - 2 + 1 / mueff) / ((N + 2) ** 2 + 2 * mueff / 2)), weights=w, neg_weights=wn,
                neg_mueff=neg_mueff, neg_cmuexp=0.3 * neg_mueff / ((N + 2) ** 1.5 + neg_mueff),
                damps=0.5 + 0.5 * min(1, (0 / (0.159 * popsize) - 1) ** 2) + 2 * max(0, ((mueff - 1) / (N + 1)) ** 0.5 - 1) + cs,
                chiN=N ** 0.5 * (1 - 1. / (4. * N) + 1. / (21. * N ** 2)), lam_mirr=0, cmean=1.0)


@pytest.mark.parametrize("N", [2, 24, 1250])
def test_constants(N):
    from rllab_amd.algos.cma_state import CMAParameters, CMAState
    g = np.load(os.path.join(GOLDEN, "cmaes_ref_constants.npz"))
    got = CMAParameters(N).as_dict()
    for k, v in got.items():
        ref = g["N%d_%s" % (N, k)]
        v = np.asarray(v, dtype=np.float64)
        if k in ("popsize", "mu", "neg_mu", "lam_mirr"):
            assert np.array_equal(v, ref), (N, k, v, ref)
        else:                                             # the same expressions; log may differ in the last bit between builds
            assert v.shape == ref.shape and np.allclose(v, ref, rtol=1e-15, atol=0), (N, k, v, ref)
    st = CMAState(torch.zeros(N, dtype=torch.float64), 1.0) if N < 100 else None
    if st is not None:
        assert st.opts["maxiter"] == float(g["N%d_maxiter" % N]) and st.opts["tolstagnation"] == int(g["N%d_tolstagnation" % N])
    restated = _np_constants(N)
    for k, v in restated.items():
        assert np.allclose(np.asarray(got[k], dtype=np.float64), v, rtol=1e-14, atol=0), (N, k)
    if N == 1250:
        assert (got["popsize"], got["mu"], got["neg_mu"]) == (25, 12, 12)
    # the fixtures of the runs carry the same constants
    if N == 24:
        r = np.load(os.path.join(GOLDEN, "cmaes_ref_plain.npz"))
        for k, v in got.items():
            assert np.allclose(np.asarray(v, dtype=np.float64), r["const_" + k], rtol=1e-15, atol=0), k
    # CMA_active off: no negative part
    off = CMAParameters(N, active=False)
    assert off.neg_mu == 0 and off.neg_cmuexp == 0 and off.c1 == got["c1"]
    with pytest.raises(NotImplementedError):
        CMAParameters(N, popsize=5)                      # the library turns mirrored sampling on below 6


def test_ask_identity():
    """xs = mean + sigma (B (D o z)) for the z of the draw, and B diag(D^2) B^T = C after an update of B and D."""
    es, _ = replay_case("wait3")
    assert es.countiter == 20 and es.itereigenupdated == 16
    xs = es.ask()                                        # iteration 20: the update is due
    assert es.itereigenupdated == 20
    z = es.last_z
    assert tuple(xs.shape) == tuple(z.shape) == (es.sp.popsize, es.N)
    want = es.mean + es.sigma * torch.matmul(es.B, (es.D * z).t()).t()
    assert torch.equal(xs, want)
    C = torch.matmul(es.B * es.D ** 2, es.B.t())
    assert float((C - es.C).abs().max() / es.C.abs().max()) <= 1e-12
    assert float((torch.matmul(es.B.t(), es.B) - torch.eye(es.N, dtype=torch.float64)).abs().max()) <= 1e-12
    assert bool((es.D[1:] >= es.D[:-1]).all())
    # the same seed draws the same points; ask(number) draws that many
    a, b = (replay_case("plain")[0] for _ in range(2))
    assert torch.equal(a.ask(7), b.ask(7)) and a.last_z.shape[0] == 7
    es.tell(xs, torch.arange(xs.shape[0], dtype=torch.float64))
    with pytest.raises(RuntimeError):                     # one tell per ask
        es.tell(xs, torch.arange(xs.shape[0], dtype=torch.float64))


@pytest.mark.parametrize("scale,clipped", [(2.0, True), (0.02, False)])
def test_negative_update_with_two_extra_eigendecompositions(scale, clipped):
    """updateBD's guarded negative update on a constructed _Yneg (cma_es_lib.py:4037-4046): the learning rate is clipped to
    clip_fac / max eig(C^-1/2 Yneg C^-1/2) when cmuexp times that eigenvalue exceeds clip_fac = 0.6, against a NumPy
    restatement of those lines; the clipped form costs one more eigendecomposition."""
    es, _ = replay_case("wait8_ask40")
    rng = np.random.RandomState(5)
    N, cmuexp = es.N, es.sp.neg_cmuexp
    A = rng.randn(N, N)
    Yneg = scale * N * (A @ A.T) / N - es.C.numpy()
    Yneg = (Yneg + Yneg.T) / 2
    es._Yneg = torch.as_tensor(Yneg.copy())
    es.itereigenupdated = es.countiter - 9                # gap 9 > updatecovwait = 8: due, and past the plain-subtraction test
    gap = 9
    assert not (gap * cmuexp * N < 0.6 * (1 - es.sp.cmu - es.sp.c1) ** gap)
    # :4037-4046 in NumPy
    C = es.C.numpy().copy()
    C = (C + C.T) / 2
    w, B = np.linalg.eigh(C)
    D = np.sqrt(w)
    inv_root = (B / D) @ B.T
    inv_root = (inv_root + inv_root.T) / 2
    eigvals = np.linalg.eigvalsh(inv_root @ Yneg @ inv_root)
    assert (eigvals.max() * cmuexp > 0.6) == clipped
    C_want = C - (cmuexp if not clipped else 0.6 / eigvals.max()) * Yneg
    before = es.count_eigen
    es.ask()
    assert es.count_eigen - before == (4 if clipped else 3)
    assert float(es._Yneg.abs().max()) == 0.0 and es.itereigenupdated == es.countiter
    C_want = (C_want + C_want.T) / 2
    assert np.abs(es.C.numpy() - C_want).max() <= 1e-12 * np.abs(C_want).max()
    if clipped:
        assert np.linalg.eigvalsh(es.C.numpy()).min() > 0     # what the clip is for
    assert np.abs(np.sort(es.D.numpy()) - np.sqrt(np.linalg.eigvalsh(C_want))).max() <= 1e-12 * es.D.numpy().max()


def _set(es, **kw):
    for k, v in kw.items():
        setattr(es, k, torch.as_tensor(v, dtype=torch.float64) if k in ("sigma", "mean", "D", "dC", "pc") else v)
    return es


def _trigger(es, key):
    """Put a fixture state where the library's default threshold of ``key`` is crossed (cma_es_lib.py:4849-4928)."""
    from rllab_amd.algos.cma_state import FLAT_FITNESS_KEY
    N = es.N
    if key == "maxiter":
        _set(es, countiter=int(es.opts["maxiter"]))
    elif key == "maxfevals":
        _set(es, countevals=float("inf"))
    elif key == "tolx":
        _set(es, sigma=1e-13)
    elif key == "tolfacupx":
        _set(es, sigma=es.sigma0 * 1e4)
    elif key == "tolfun":
        _set(es, fit_hist=[1.0, 1.0 + 1e-13, 1.0], _fit_first=1.0, _fit_last=1.0 + 1e-13)
    elif key == "tolfunhist":
        _set(es, fit_hist=[1.0 + 1e-14 * i for i in range(10)])
    elif key == "tolstagnation":
        _set(es, countiter=int(N * (5 + 100 / es.sp.popsize)) + 1, fit_histbest=[1.0] * 250, fit_histmedian=[2.0] * 250)
    elif key == "tolupsigma":
        _set(es, sigma=es.sigma0 * 1e21)
    elif key == "noeffectcoord":
        m = es.mean.clone()
        m[3] = 1e20
        _set(es, mean=m)
    elif key == "noeffectaxis":
        _set(es, mean=torch.full((N,), 1e20))
    elif key == "conditioncov":
        d = es.D.clone()
        d[-1] = 1.1e7 * d[0]
        _set(es, D=d)
    elif key == FLAT_FITNESS_KEY:
        _set(es, fit_hist=[3.0] * 10)                     # tolfunhist fires with it: the entry needs another one
    else:
        raise KeyError(key)


def test_stop_criteria():
    from rllab_amd.algos.cma_state import FLAT_FITNESS_KEY, CMAState
    keys = ["maxiter", "maxfevals", "tolx", "tolfacupx", "tolfun", "tolfunhist", "tolstagnation", "tolupsigma",
            "noeffectcoord", "noeffectaxis", "conditioncov", FLAT_FITNESS_KEY]
    assert CMAState(torch.zeros(4, dtype=torch.float64), 1.0).stop() == {}          # before the first tell
    for key in keys:
        es, _ = replay_case("plain")
        assert es.stop() == {}, key                       # silent on the fixture state
        _trigger(es, key)
        fired = es.stop()
        assert key in fired, (key, fired)
    # the thresholds are the library's defaults
    es, _ = replay_case("plain")
    o = es.opts
    assert (o["tolx"], o["tolfun"], o["tolfunhist"], o["tolfacupx"], o["tolupsigma"]) == (1e-11, 1e-11, 1e-12, 1e3, 1e20)
    assert o["maxiter"] == 100 + 50 * (24 + 3) ** 2 // 13 ** 0.5 and o["tolstagnation"] == int(100 + 100 * 24 ** 1.5 / 13)
    # an index list is "any" only with a nonzero index in it (:4894-4896): coordinate 0 alone does not stop
    m = es.mean.clone()
    m[0] = 1e20
    assert "noeffectcoord" not in _set(es, mean=m).stop()
    # where the library would introduce a transform (max D / min D > 1e6 at an update of B and D), the state stops
    es, _ = replay_case("plain")
    es.C = es.C.clone()
    es.C[0, 0] *= 1e13
    es.ask()
    assert "conditioncov" in es.stop()
    with pytest.raises(TypeError):
        CMAState(torch.zeros(4, dtype=torch.float64), 1.0, dict(bounds=[0, 1]))


def test_sigma_guards_and_rescale():
    """minstd / maxstd / mindx act on sigma after the step-size update; sigma > 1e9 sigma0 moves the scale into C."""
    from rllab_amd.algos.cma_state import CMAState
    g = np.load(os.path.join(GOLDEN, "cmaes_ref_plain.npz"))
    lam = int(g["lam"][0])

    def one_tell(options, sigma=None):
        es = CMAState(torch.as_tensor(g["x0"]), float(g["sigma0"]), dict(options, seed=1))
        es.ask()
        if sigma is not None:
            es.sigma = torch.as_tensor(sigma, dtype=torch.float64)
        es.tell(torch.as_tensor(g["xs"][:lam]), torch.as_tensor(g["fs"][:lam]))
        return es
    base = one_tell({})
    assert abs(float(base.sigma) - float(g["sigma"][0])) <= PARITY_TOL * float(g["sigma"][0])
    es = one_tell(dict(minstd=5.0))
    assert abs(float(es.sigma * (es.dC ** 0.5).min()) - 5.0) <= 1e-12
    es = one_tell(dict(maxstd=0.01))
    assert abs(float(es.sigma * (es.dC ** 0.5).max()) - 0.01) <= 1e-14
    es = one_tell(dict(mindx=7.0))
    assert abs(float(es.sigma * es.D.min()) - 7.0) <= 1e-12
    big = one_tell({}, sigma=1e12)
    # alpha = sigma / max D;  C *= alpha, D *= sqrt(alpha), sigma /= sqrt(alpha): the sampled distribution keeps sigma^2 C
    assert float(big.sigma) < 1e9 * big.sigma0 * 1e-2 and float(big.tolupsigma) < 1e20
    assert float(big.C.diagonal().min()) > 1e6 and torch.equal(big.dC, big.C.diagonal())


def test_cov_update_definition():
    """cov_update_torch against cma_es_lib.py:3808-3814 restated in NumPy."""
    from rllab_amd.algos.cma_state import cov_update_torch
    rng = np.random.RandomState(2)
    N, mu, mun = 17, 5, 4
    A = rng.randn(N, N)
    C = A @ A.T / N
    Yn = rng.randn(N, N)
    Yn = Yn + Yn.T
    Y, V, pc = rng.randn(mu, N), rng.randn(mun, N), rng.randn(N)
    wp, wn = rng.rand(mu) * 0.1, rng.rand(mun)
    scal = np.array([0.93, 0.004, 0.99])
    Yn_want = Yn * scal[2] + (np.dot(wn * V.T, V) - C)
    C_want = C * scal[0] + (np.outer(scal[1] * pc, pc) + np.dot(wp * Y.T, Y))
    t = torch.as_tensor
    Ct, Ynt, dC = t(C.copy()), t(Yn.copy()), torch.zeros(N, dtype=torch.float64)
    cov_update_torch(Ct, Ynt, dC, t(Y), t(wp), t(V), t(wn), t(pc), t(scal))
    assert np.abs(Ct.numpy() - C_want).max() <= 1e-14 and np.abs(Ynt.numpy() - Yn_want).max() <= 1e-14
    assert np.array_equal(dC.numpy(), np.diag(Ct.numpy()))
    C2, dC2 = t(C.copy()), torch.zeros(N, dtype=torch.float64)
    cov_update_torch(C2, None, dC2, t(Y), t(wp), None, None, t(pc), t(scal))
    assert torch.equal(C2, Ct)


def test_constructor_has_the_reference_signature():
    from rllab_amd.algos.cma_es import CMAES
    p = inspect.signature(CMAES.__init__).parameters
    want = [("n_itr", 500), ("max_path_length", 500), ("discount", 0.99), ("sigma0", 1.), ("batch_size", None), ("plot", False)]
    assert list(p)[:3] == ["self", "env", "policy"]
    assert [(k, p[k].default) for k in list(p)[3:3 + len(want)]] == want                # rllab/algos/cma_es.py:32-43
    assert p["popsize"].default is None and p["seed"].default is None and p["record_paths"].default is True
    assert p["updatecovwait"].default is None and p["active"].default is True
    assert list(p)[-1] == "kwargs" and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # engine options survive the constructor-argument pickle
    import pickle
    a = CMAES(env=None, policy=None, n_itr=3, popsize=64, updatecovwait=2, active=False)
    b = pickle.loads(pickle.dumps(a))
    assert (b.n_itr, b.popsize, b.updatecovwait, b.active) == (3, 64, 2, False)


def test_importable_under_the_reference_path():
    """``rllab.algos.cma_es.CMAES`` resolves through the alias package (the module this change adds)."""
    import rllab.algos.cma_es as aliased
    from rllab_amd.algos.cma_es import CMAES
    assert aliased.CMAES is CMAES


def test_cov_update_abi():
    from rllab_amd import _lib
    text = open(os.path.join(ROOT, "include", "rllab_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int rl_cmaes_cov_update\((.*?)\);", text, flags=re.S)
    assert m and "rl_cmaes_cov_update" in _lib.SYMBOLS
    assert len(m.group(1).split(",")) == len(_lib.lib.rl_cmaes_cov_update.argtypes) == 14
    # argument errors come back as codes, nothing is launched
    assert _lib.lib.rl_cmaes_cov_update(0, 0, 1, 0, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"rl_cmaes_cov_update" in _lib.lib.rl_last_error()
    assert "lib.rl_cmaes_cov_update.argtypes" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_shared_refusal_function():
    """CEM and CMAES ask the same function; CMAES adds the size limit of the full covariance."""
    from rllab_amd.algos import cem, cma_es
    assert cma_es.population_why_unsupported is cem.population_why_unsupported
    src = inspect.getsource(cma_es.CMAES.why_unsupported)
    assert "population_why_unsupported" in src and cma_es.MAX_PARAMS == 8192
    assert "plot=True" in cem.population_why_unsupported(None, None, plot=True)


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout the fixtures are made from")
def test_fixture_regenerates():
    """One case run again through the reference's library (in memory): constants and points equal, states to 1e-12."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_cmaes", os.path.join(ROOT, "tools", "make_golden_cmaes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new = mod.run_case(mod.load_library("/root/reference"), "wait3")
    old = np.load(os.path.join(GOLDEN, "cmaes_ref_wait3.npz"))
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        a, b = np.asarray(new[k]), old[k]
        if k.startswith("const_") or k in ("x0", "sigma0", "n_itr", "lam", "count_eigen", "stop", "eig_per_ask", "C_iters",
                                            "option_names", "option_values"):
            assert np.array_equal(a, b), k
        else:
            assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0), k
