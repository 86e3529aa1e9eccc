"""rl_reps_dual / rl_reps_weights (csrc/reps_kernels.hip) against the float64 torch definition of
rllab_amd/algos/reps.py on the same float32 planes; the log-likelihood value + gradient pass LbfgsOptimizer uses for
VPG / ERWR / REPS; one REPS iteration on the kernels against the same iteration on the definition; ERWR and REPS
learning Cartpole; the two examples.

Tolerances: 1e-5 relative on the dual, 1e-5 of the gradient's largest component on every component (float32
post-processing against float64: the repository's standing "within 1e-5"), 1e-5 absolute on the weights (they lie in
[0, 1])."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.5


def _native_widths():
    from rllab_amd import _lib
    return sorted({_lib.env_query(k)["obs_dim"] for k in range(8)})


def _synthetic(Do, T, N, seed, p_done=0.03):
    """Ragged planes on the device: random done flags (several paths per column), the trailing incomplete paths cut from
    the batch (invalid tails), observations beyond +-10."""
    from rllab_amd.sampler.trajectories import Trajectories
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    obs = torch.randn(Do, T, N, device=dev, generator=g) * 4.0
    rewards = torch.randn(T, N, device=dev, generator=g)
    dones = (torch.rand(T, N, device=dev, generator=g) < p_done).to(torch.uint8)
    dones[T - 1, ::3] = 1                       # a third of the columns end on a done flag: no invalid tail there
    if N > 1:
        dones[:, 1] = 0                         # a column without any done flag: all of it is cut ...
    traj = Trajectories(obs, torch.zeros((1, T, N), device=dev), torch.zeros((1, T, N), device=dev),
                        torch.zeros(1, device=dev), rewards, dones, T)
    traj.valid = traj.valid_mask(whole_paths=True)
    if N > 2:
        traj.valid[:, 2] = True                 # ... and one kept whole although its last path is cut by the horizon
    traj.tin = traj.time_in_path().to(torch.int32)
    return traj


def _check(traj, eta, v, label=""):
    """Kernel sums -> dual / gradient / weights against the definition; returns the printed figures."""
    from rllab_amd.algos import reps as R
    assert R.FusedRepsDual.accepts(traj)
    k = R.FusedRepsDual(traj)
    sums = k.sums(eta, v)
    out1 = k.out.clone()
    w = k.weights(eta, v)
    # the definition, float64, on the same float32 planes
    fd = R.reps_feat_diff(traj.obs, traj.tin, traj.dones, traj.valid)
    want, want_g = R.reps_dual(eta, v, traj.rewards, fd, traj.valid, EPS, 1e-5)
    want_w = R.reps_weights(eta, v, traj.rewards, fd, traj.valid)
    got, got_g = R.dual_from_sums(eta, sums, EPS, 1e-5)
    assert np.all(np.isfinite(sums)) and np.isfinite(got) and np.all(np.isfinite(got_g))
    assert sums[3] == float(traj.valid.sum())
    e_val = abs(got - want) / abs(want)
    e_grad = np.abs(got_g - want_g).max() / np.abs(want_g).max()
    e_w = float((w.double() - want_w).abs().max())
    print("reps %s T=%d N=%d Do=%d eta=%g |v|=%.3g: dual %.9g (rel err %.2e) grad err %.2e weights err %.2e"
          % (label, traj.T, traj.N, traj.obs_dim, eta, np.abs(v).max(), got, e_val, e_grad, e_w))
    assert e_val <= 1e-5 and e_grad <= 1e-5 and e_w <= 1e-5
    assert bool((w[~traj.valid.bool()] == 0).all()) and float(w.max()) <= 1.0
    # two launches on the same inputs: bit-identical
    k2 = R.FusedRepsDual(traj)
    k2.launch(eta, v)
    assert torch.equal(k2.out, out1)
    assert torch.equal(k2.weights(eta, v), w) and torch.equal(k2.out, out1)
    return e_val, e_grad, e_w


def _v(d, mag, seed):
    return mag * np.random.RandomState(seed).randn(d)


def test_every_native_observation_width():
    widths = _native_widths()
    assert set([4, 6, 11, 13, 20, 21]) <= set(widths)
    for i, Do in enumerate(widths + [30]):
        traj = _synthetic(Do, 50, 257, seed=i)
        _check(traj, 15.0, _v(2 * Do + 4, 1.0, i), "width")


@pytest.mark.parametrize("Do,T,N", [(4, 1, 1), (13, 7, 37), (6, 64, 64), (11, 129, 1000), (13, 500, 4096), (20, 500, 1024),
                                     (21, 500, 4096)])
def test_shapes_from_a_partial_tile_to_the_headline(Do, T, N):
    traj = _synthetic(Do, T, N, seed=T + N, p_done=0.03 if T < 200 else 0.004)
    _check(traj, 15.0, _v(2 * Do + 4, 1.0, 3), "shape")
    _check(traj, 0.05, _v(2 * Do + 4, 10.0, 4), "shape")


@pytest.mark.parametrize("Do", [6, 20])
def test_sharp_and_flat_soft_max(Do):
    """eta from 1e-2 (delta / eta reaches 1e5: nothing may overflow or turn NaN) to 1e3, |v| from 1e-3 to 1e1."""
    traj = _synthetic(Do, 100, 512, seed=7)
    for eta in (1e-2, 1e-1, 1.0, 15.0, 1e3):
        for mag in (1e-3, 1.0, 10.0):
            _check(traj, eta, _v(2 * Do + 4, mag, 11), "eta/v")


def _algo(cls, env_name, n_envs, horizon, seed, hidden=(32, 32), **kw):
    from rllab_amd.baselines.linear_feature_baseline import LinearFeatureBaseline
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(seed)
    if env_name == "cartpole":
        from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
        env = normalize(CartpoleEnv())
    else:
        from rllab_amd.envs.mujoco.swimmer_env import SwimmerEnv
        env = normalize(SwimmerEnv())
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=hidden)
    algo = cls(env=env, policy=policy, baseline=LinearFeatureBaseline(env_spec=env.spec), batch_size=n_envs * horizon,
               max_path_length=horizon, discount=0.99, sampler_args=dict(n_envs=n_envs, seed=seed), **kw)
    return algo


@pytest.mark.parametrize("env_name,n_envs,horizon", [("cartpole", 256, 100), ("swimmer", 128, 500)])
def test_real_rollouts(env_name, n_envs, horizon, quiet_logger):
    """Ragged paths of a terminating env (Cartpole: several paths per column, invalid tails) and full-length ones of an
    env that never terminates (Swimmer)."""
    from rllab_amd.algos.reps import REPS
    algo = _algo(REPS, env_name, n_envs, horizon, seed=3, n_itr=1)
    algo.start_worker()
    algo.init_opt()
    sd = algo.sampler.process_samples(0, algo.sampler.obtain_samples(0))
    traj = sd["_traj"]
    if env_name == "cartpole":
        assert not bool(traj.valid.all()) and int(traj.dones.sum()) > n_envs
    else:
        assert bool(traj.valid.all()) and int(traj.dones.sum()) == n_envs
    d = 2 * traj.obs_dim + 4
    for eta, mag in ((15.0, 1.0), (1e-2, 10.0), (1e3, 1e-3)):
        _check(traj, eta, np.abs(_v(d, mag, 5)), env_name)
    algo.shutdown_worker()


@pytest.mark.parametrize("h", [32, 64])
def test_value_and_grad_of_the_log_likelihood_objective(h):
    """FusedGaussianMLPOps.value_and_grad(vpg=True) and loglik_loss against float64 autograd of
    -sum(w logli adv) * inv_count (tolerances of tests/test_gpu_update_parity.py's vpg checks)."""
    from tests.test_gpu_update_parity import _closures, _inputs, _policy
    for do, da in ((13, 2), (20, 6)):
        pol = _policy(do, da, h)
        ops = pol.fused_ops()
        inp = _inputs(pol, 70001)
        _, _, vpg = _closures(pol)
        flat64 = pol.flat_params.detach().double().requires_grad_(True)
        v64 = vpg(flat64, *inp)
        g64 = torch.autograd.grad(v64, flat64)[0].cpu().numpy()
        val, g = ops.value_and_grad(inp, vpg=True)
        v64f = float(v64.detach())
        assert abs(val - v64f) <= 2e-5 * max(1.0, abs(v64f))
        assert np.abs(g - g64).max() <= 2e-5 * max(1e-3, np.abs(g64).max())
        assert abs(ops.loglik_loss(inp) - v64f) <= 2e-5 * max(1.0, abs(v64f))
        # the default is untouched: the likelihood-ratio surrogate, a different function away from old == new
        val0, g0 = ops.value_and_grad(inp)
        assert abs(val0 - (-ops.loss_stats_host(inp)[0])) <= 1e-12 * max(1.0, abs(val0))
        assert np.abs(g0 - g).max() > 1e-3 * np.abs(g).max()


@pytest.mark.parametrize("env_name,n_envs,horizon", [("cartpole", 4096, 100), ("swimmer", 4096, 500)])
def test_reps_iteration_on_the_kernels_against_the_definition(env_name, n_envs, horizon, quiet_logger):
    """One REPS iteration from the same seed on the same batch, with the kernels and with ``use_fused = False``:
    DualBefore and DualAfter agree to 1e-5 relative (the optimum's value is stable where its argument is not)."""
    from rllab_amd.algos.reps import REPS
    from rllab_amd.misc import logger
    algo = _algo(REPS, env_name, n_envs, horizon, seed=5, n_itr=1)
    algo.start_worker()
    algo.init_opt()
    assert algo._fused is not None
    sd = algo.sampler.process_samples(0, algo.sampler.obtain_samples(0))
    theta0 = algo.policy.get_param_values()
    eta0, v0 = algo.param_eta, algo.param_v.copy()
    algo.optimize_policy(0, sd)
    fused = {k: float(v) for k, v in logger.get_tabular().items() if k in ("DualBefore", "DualAfter", "LossBefore",
                                                                           "LossAfter", "MeanKL")}
    logger.dump_tabular()
    ref = REPS(env=algo.env, policy=algo.policy, baseline=algo.baseline, sampler_cls=lambda a: None)
    ref.use_fused = False
    ref.init_opt()
    assert ref._fused is None
    ref.param_eta, ref.param_v = eta0, v0.copy()
    algo.policy.set_param_values(theta0)
    ref.optimize_policy(0, sd)
    plain = {k: float(v) for k, v in logger.get_tabular().items() if k in fused}
    logger.dump_tabular()
    print("reps iteration %s: kernels %r definition %r eta %g / %g" % (env_name, fused, plain, algo.param_eta, ref.param_eta))
    assert all(np.isfinite(v) for v in fused.values()) and fused["DualAfter"] <= fused["DualBefore"]
    for key in ("DualBefore", "DualAfter"):
        assert abs(fused[key] - plain[key]) <= 1e-5 * abs(plain[key]), (key, fused[key], plain[key])
    algo.shutdown_worker()


@pytest.mark.parametrize("name", ["erwr", "reps"])
def test_erwr_and_reps_learn_cartpole(name, quiet_logger, tmp_path):
    """A fixed small number of iterations on normalize(CartpoleEnv()): every logged value finite, the mean AverageReturn
    of the last three iterations above that of the first three."""
    from rllab_amd.algos.erwr import ERWR
    from rllab_amd.algos.reps import REPS
    from rllab_amd.misc import logger
    n_itr = 12
    algo = _algo(ERWR if name == "erwr" else REPS, "cartpole", 256, 100, seed=1, n_itr=n_itr)
    algo.start_worker()
    algo.init_opt()
    rets = []
    for itr in range(n_itr):
        paths = algo.sampler.obtain_samples(itr)
        sd = algo.sampler.process_samples(itr, paths)
        algo.log_diagnostics(paths)
        algo.optimize_policy(itr, sd)
        tab = logger.get_tabular()
        for k, v in tab.items():
            assert np.isfinite(float(v)), (itr, k, v)
        rets.append(float(tab["AverageReturn"]))
        logger.dump_tabular()
    algo.shutdown_worker()
    print("%s cartpole AverageReturn: %s" % (name, " ".join("%.1f" % r for r in rets)))
    assert np.isfinite(algo.policy.get_param_values()).all()
    assert np.mean(rets[-3:]) > np.mean(rets[:3]), rets


@pytest.mark.parametrize("script", ["erwr_cartpole.py", "reps_cartpole.py"])
def test_examples_run_verbatim(script, tmp_path):
    """The example as a user starts it (a fresh process, its own defaults); --csv only adds the log this test reads."""
    csv_path = str(tmp_path / "progress.csv")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), "--csv", csv_path], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    import csv
    rows = list(csv.DictReader(open(csv_path)))
    assert len(rows) == 15
    assert all(np.isfinite(float(x["AverageReturn"])) and np.isfinite(float(x["LossAfter"])) for x in rows)
    if script.startswith("reps"):
        assert all(float(x["DualAfter"]) <= float(x["DualBefore"]) for x in rows)
