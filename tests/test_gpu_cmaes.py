"""CMA-ES on the device: rl_cmaes_cov_update against its torch definition, CMAState replaying the reference library's
fixtures with its state on the MI355X, and CMAES (rllab/algos/cma_es.py) end to end on the population rollout."""
import csv
import os

import numpy as np
import pytest
import torch

from tests.test_cmaes_host import CASES, PARITY_TOL, replay_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _cov_inputs(N, mu, mu_neg, seed):
    rng = np.random.RandomState(seed)
    A = rng.randn(N, N)
    C = A @ A.T / N + np.eye(N)
    Yn = rng.randn(N, N)
    Yn = Yn + Yn.T
    return dict(C=C, Yneg=Yn, Ypos=rng.randn(mu, N), wpos=rng.rand(mu) / mu, Vneg=rng.randn(mu_neg, N),
                wneg=rng.rand(mu_neg) / max(mu_neg, 1), pc=rng.randn(N), scal=np.array([0.93, 0.004, 0.99]))


def _launch(inp, active, pad=(3, 5)):
    """The kernel on the N x N corner of a padded allocation filled with a sentinel -> (C, Yneg, dC, the allocations)."""
    from rllab_amd.algos.cma_state import cov_update_hip
    N = inp["C"].shape[0]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    bufs = []
    for name in ("C", "Yneg"):
        buf = torch.full((N + pad[0], N + pad[1]), -777.0, dtype=torch.float64, device=DEV)
        buf[:N, :N] = t(inp[name])
        bufs.append(buf)
    dC = torch.full((N + 2,), -777.0, dtype=torch.float64, device=DEV)
    Cv, Yv = bufs[0][:N, :N], bufs[1][:N, :N]
    cov_update_hip(Cv, Yv if active else None, dC, t(inp["Ypos"]), t(inp["wpos"]), t(inp["Vneg"]) if active else None,
                   t(inp["wneg"]) if active else None, t(inp["pc"]), t(inp["scal"]))
    torch.cuda.synchronize()
    return Cv, Yv, dC, bufs


# (N, mu, mu_neg): below one tile; one tile row and a bit; two column tiles with more negative ranks than a chunk of 32;
# several tiles each way with both rank loops running three chunks
@pytest.mark.parametrize("N,mu,mu_neg", [(5, 1, 0), (33, 6, 6), (70, 3, 40), (130, 70, 70)])
def test_cov_update_kernel(N, mu, mu_neg):
    from rllab_amd.algos.cma_state import cov_update_torch
    active = mu_neg > 0                                   # (5, 1, 0): NULL negative arguments
    inp = _cov_inputs(N, mu, mu_neg, seed=N)
    Cv, Yv, dC, bufs = _launch(inp, active)
    # the definition, in torch float64 on the host
    t = torch.as_tensor
    C_ref, Y_ref, dC_ref = t(inp["C"].copy()), t(inp["Yneg"].copy()), torch.zeros(N, dtype=torch.float64)
    cov_update_torch(C_ref, Y_ref if active else None, dC_ref, t(inp["Ypos"]), t(inp["wpos"]),
                     t(inp["Vneg"]) if active else None, t(inp["wneg"]) if active else None, t(inp["pc"]), t(inp["scal"]))
    # per entry: relative 4 (mu + mu_neg + 2) 2^-53 of the largest summand magnitude (derived from the length of the sums
    # and the unit roundoff, not measured)
    rel = 4 * (mu + mu_neg + 2) * 2.0 ** -53
    s = inp["scal"]
    big_C = np.maximum(np.abs(s[0] * inp["C"]), np.abs(s[1] * np.outer(inp["pc"], inp["pc"])))
    big_C = np.maximum(big_C, np.abs(inp["wpos"][:, None, None] * inp["Ypos"][:, :, None] * inp["Ypos"][:, None, :]).max(axis=0))
    err_C = np.abs(Cv.cpu().numpy() - C_ref.numpy())
    print("rl_cmaes_cov_update N=%d mu=%d mu_neg=%d: C max err / bound = %.3f" % (N, mu, mu_neg, (err_C / (rel * big_C)).max()))
    assert (err_C <= rel * big_C).all()
    assert torch.equal(Cv, Cv.t())                        # exactly symmetric
    assert torch.equal(dC[:N], torch.diagonal(Cv))
    if active:
        big_Y = np.maximum(np.abs(s[2] * inp["Yneg"]), np.abs(inp["C"]))
        big_Y = np.maximum(big_Y, np.abs(inp["wneg"][:, None, None] * inp["Vneg"][:, :, None] * inp["Vneg"][:, None, :]).max(axis=0))
        err_Y = np.abs(Yv.cpu().numpy() - Y_ref.numpy())
        print("   _Yneg max err / bound = %.3f" % (err_Y / (rel * big_Y)).max())
        assert (err_Y <= rel * big_Y).all()
        assert torch.equal(Yv, Yv.t())
    else:
        assert torch.equal(Yv.cpu(), t(inp["Yneg"]))      # not touched
    # nothing outside the N x N corner (or past dC[N]) was written
    for buf in bufs:
        assert bool((buf[N:, :] == -777.0).all()) and bool((buf[:, N:] == -777.0).all())
    assert bool((dC[N:] == -777.0).all())
    # a second launch on equal inputs: equal bits
    C2, Y2, dC2, _ = _launch(inp, active)
    assert torch.equal(C2, Cv) and torch.equal(Y2, Yv) and torch.equal(dC2, dC)


@pytest.mark.parametrize("case", CASES)
def test_replay_parity_on_device(case):
    es, worst = replay_case(case, device=DEV)
    print("replay %s (device): %s" % (case, {k: "%.2e" % v for k, v in worst.items()}))
    assert es.C.is_cuda and es.B.is_cuda
    assert max(worst.values()) <= PARITY_TOL, worst


KEYS = ["Iteration", "CurStdMean", "AverageReturn", "StdReturn", "MaxReturn", "MinReturn", "AverageDiscountedReturn",
        "AvgTrajLen", "Sigma", "AxisRatio", "NumTrajs"]


def _train(tmp_path, name, hidden=(8,), **kw):
    from rllab.algos.cma_es import CMAES
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import ext, logger
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(kw.get("seed", 1))
    env = normalize(CartpoleEnv())
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=hidden)
    algo = CMAES(env=env, policy=policy, **kw)
    path = str(tmp_path / (name + ".csv"))
    logger.add_tabular_output(path)
    try:
        algo.train()
    finally:
        logger.remove_tabular_output(path)
    with open(path) as f:
        reader = csv.DictReader(f)
        rows = list(reader)
        header = reader.fieldnames
    return algo, policy, header, rows


@pytest.mark.parametrize("batch_size", [1000, None])
def test_cmaes_end_to_end(tmp_path, quiet_logger, batch_size):
    """The arguments of the reference's algorithm matrix (tests/test_algos.py:76-94: batch_size=1000, max_path_length=100,
    n_itr=... here 3) and the same without batch_size."""
    kw = dict(n_itr=3, max_path_length=100, batch_size=batch_size, seed=1)
    algo, policy, header, rows = _train(tmp_path, "a", **kw)
    assert header[:len(KEYS)] == KEYS and len(rows) == 3
    assert [int(r["Iteration"]) for r in rows] == [0, 1, 2]
    assert all(float(r["CurStdMean"]) == 1.0 for r in rows)                      # the reference logs sigma0
    assert all(r["StdReturn"] == r["AverageReturn"] for r in rows)               # ... and the mean as StdReturn
    assert "AveragePolicyStd" in header
    theta = policy.get_param_values()
    assert np.all(np.isfinite(theta))
    es = algo.es
    popsize = 4 + int(3 * np.log(theta.size))
    assert es.sp.popsize == popsize and es.countiter == 3 and es.countevals == 3 * popsize
    if batch_size is None:
        assert all(int(float(r["NumTrajs"])) == popsize for r in rows)
    else:
        from rllab_amd.algos.cem import cem_sample_prefix
        lengths = algo.last_lengths.cpu().numpy()
        assert lengths.size % 10 == 0                       # launches of ceil(1000 / 100) candidates
        used = cem_sample_prefix(lengths, 1000)
        assert used == algo.last_n_candidates == algo.last_xs.shape[0] == int(float(rows[-1]["NumTrajs"]))
        assert cem_sample_prefix(lengths[:lengths.size - 10], 1000) is None
        print("batch_size=1000: %d candidates launched, %d told (popsize %d)" % (lengths.size, used, popsize))
        assert used >= 10
    # the final parameters are the best-ever evaluated candidate
    assert len(algo.iteration_best) == 3
    fs = torch.stack([f for f, _ in algo.iteration_best]).cpu().numpy()
    best_x = algo.iteration_best[int(np.argmin(fs))][1]
    assert np.array_equal(theta.astype(np.float32), best_x.to(torch.float32).cpu().numpy())
    assert es.result()[1] == fs.min()
    i_last = int(torch.sort(algo.last_fs, stable=True).indices[0])
    assert torch.equal(algo.iteration_best[-1][1], algo.last_xs[i_last])
    assert abs(float(rows[-1]["AverageDiscountedReturn"]) - float(algo.last_fs.mean())) <= 1e-9
    # the same seed again: equal parameters, bit for bit
    _, policy2, header2, rows2 = _train(tmp_path, "b", **kw)
    assert np.array_equal(policy2.get_param_values(), theta) and rows2 == rows and header2 == header


# oracle: tools/exp/cmaes_cpu_curves.py -- the same CMAState loop on the CPU (host env in float64, float64 numpy policy),
# seeds 1..5, hidden_sizes=(8,), max_path_length=100, popsize=64, sigma0=0.5: profiles/curves/cmaes_cartpole_cpu.csv
LEARN_N_ITR = 2           # the smallest n_itr at which all five CPU seeds gain (popsize 64 sufficed: no need for 256)
LEARN_MIN_CPU_GAIN = 1.0935451108337872    # (seed 1: 33.9 -> 35.0) the smallest gain of AverageReturn, iteration 0 -> iteration LEARN_N_ITR - 1, over the five seeds


def _cpu_gains(n_itr):
    curves = {}
    with open(os.path.join(ROOT, "profiles", "curves", "cmaes_cartpole_cpu.csv")) as f:
        for r in csv.DictReader(f):
            curves.setdefault(int(r["Seed"]), {})[int(r["Iteration"])] = float(r["AverageReturn"])
    return {s: c[n_itr - 1] - c[0] for s, c in curves.items()}


def test_cmaes_learns_cartpole(tmp_path, quiet_logger):
    """AverageReturn must gain, from iteration 0 to the last, half of what the weakest of five CPU seeds gains over the
    same iterations (CEM's rule: the env arithmetic and the draws differ, the algorithm does not)."""
    gains = _cpu_gains(LEARN_N_ITR)
    assert len(gains) == 5 and min(gains.values()) > 0
    assert abs(min(gains.values()) - LEARN_MIN_CPU_GAIN) <= 1e-6        # the number quoted above is the file's
    for n_itr in range(2, LEARN_N_ITR):
        assert min(_cpu_gains(n_itr).values()) <= 0, "a smaller n_itr at which every CPU seed gains: %d" % n_itr
    _, _, _, rows = _train(tmp_path, "learn", n_itr=LEARN_N_ITR, max_path_length=100, popsize=64, sigma0=0.5, seed=1,
                           record_paths=False)
    gain = float(rows[-1]["AverageReturn"]) - float(rows[0]["AverageReturn"])
    print("CMAES on Cartpole: AverageReturn %s, gain %.2f (CPU seeds: min gain %.2f)" % (
        [round(float(r["AverageReturn"]), 1) for r in rows], gain, LEARN_MIN_CPU_GAIN))
    assert gain >= 0.5 * LEARN_MIN_CPU_GAIN


@pytest.mark.parametrize("case,word", [("wide", "hidden_sizes"), ("rectify", "rectify"), ("adaptive_std", "adaptive_std"),
                                       ("normalize_obs", "normalize_obs"), ("too_many", "8192")])
def test_cmaes_refusals(case, word):
    from rllab_amd.algos.cma_es import CMAES
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    env = normalize(CartpoleEnv(), normalize_obs=(case == "normalize_obs"))
    kw = dict(wide=dict(hidden_sizes=(100, 50, 25)), rectify=dict(hidden_nonlinearity=rectify),
              adaptive_std=dict(adaptive_std=True), normalize_obs=dict(), too_many=dict(hidden_sizes=(128, 64)))[case]
    policy = GaussianMLPPolicy(env_spec=env.spec, **kw)
    if case == "too_many":
        assert policy.get_param_values().size > 8192
    with pytest.raises(NotImplementedError) as e:
        CMAES(env=env, policy=policy, n_itr=1, max_path_length=10).train()
    assert word in str(e.value), str(e.value)
