"""ERWR and REPS on the host: import paths and signatures, the torch definition of the REPS dual against an
independent float64 numpy restatement of rllab/algos/reps.py (loops over paths, explicit zero row, np.vstack, the
literal max-subtracted expressions), one REPS iteration on CPU tensors, and which objective LbfgsOptimizer asks a
fused object for."""
import inspect

import numpy as np
import pytest
import torch


def _spec(do, da):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Box
    return EnvSpec(Box(-np.ones(do), np.ones(do)), Box(-np.ones(da), np.ones(da)))


class _Env(object):
    """The little of an env that an algorithm's constructor and init_opt read."""

    def __init__(self, do, da):
        self.spec = _spec(do, da)
        self.observation_space, self.action_space = self.spec.observation_space, self.spec.action_space


class _NoSampler(object):
    def __init__(self, algo):
        pass


def test_import_paths_and_constructor_defaults():
    import scipy.optimize
    import rllab.algos.erwr as e1
    import rllab.algos.reps as r1
    import rllab_amd.algos.erwr as e2
    import rllab_amd.algos.reps as r2
    from rllab.algos.erwr import ERWR
    from rllab.algos.reps import REPS
    from rllab_amd.algos.batch_polopt import BatchPolopt
    from rllab_amd.algos.vpg import VPG
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.optimizers.lbfgs_optimizer import LbfgsOptimizer
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    assert e1 is e2 and r1 is r2
    assert issubclass(ERWR, VPG) and issubclass(REPS, BatchPolopt)
    # rllab/algos/erwr.py:19-24
    sig = inspect.signature(ERWR.__init__).parameters
    assert [sig[k].default for k in ("optimizer", "optimizer_args", "positive_adv")] == [None, None, None]
    # rllab/algos/reps.py:23-30
    sig = inspect.signature(REPS.__init__).parameters
    assert [sig[k].default for k in ("epsilon", "L2_reg_dual", "L2_reg_loss", "max_opt_itr")] == [0.5, 0., 0., 50]
    assert sig["optimizer"].default is scipy.optimize.fmin_l_bfgs_b
    env = _Env(3, 2)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(8, 8))
    algo = ERWR(env=env, policy=pol, baseline=ZeroBaseline(env.spec), sampler_cls=_NoSampler)
    assert algo.positive_adv is True and isinstance(algo.optimizer, LbfgsOptimizer)
    algo = ERWR(env=env, policy=pol, baseline=ZeroBaseline(env.spec), sampler_cls=_NoSampler, positive_adv=False,
                optimizer_args=dict(max_opt_itr=3))
    assert algo.positive_adv is False and algo.optimizer._max_opt_itr == 3
    algo = REPS(env=env, policy=pol, baseline=ZeroBaseline(env.spec), sampler_cls=_NoSampler)
    assert (algo.epsilon, algo.L2_reg_dual, algo.L2_reg_loss, algo.max_opt_itr) == (0.5, 0., 0., 50)
    algo.init_opt()
    assert algo.param_eta == 15. and algo.param_v.shape == (2 * 3 + 4,)
    assert np.all((algo.param_v >= 0) & (algo.param_v < 1))


# ---- the numpy restatement -------------------------------------------------------------------------------------------
def _np_features(path_obs):
    """reps.py:207-211 on one path's [L, Do] observations."""
    o = np.clip(path_obs, -10, 10)
    L = len(path_obs)
    al = np.arange(L).reshape(-1, 1) / 100.0
    return np.concatenate([o, o ** 2, al, al ** 2, al ** 3, np.ones((L, 1))], axis=1)


def _np_paths(dones, valid):
    """(column, t0, t1 exclusive) of every path of the batch: maximal runs of valid steps of a column that end at a done
    flag or at the column's last valid step."""
    T, N = dones.shape
    out = []
    for n in range(N):
        t0 = 0
        for t in range(T):
            if not valid[t, n]:
                if t > t0:
                    out.append((n, t0, t))
                t0 = t + 1
                continue
            if dones[t, n] or t == T - 1:
                out.append((n, t0, t + 1))
                t0 = t + 1
    return out


def _np_batch(obs, rewards, dones, valid):
    """Flat rewards, feature rows and feature differences in path order (reps.py:228-238), with the (t, n) of each row."""
    feats, fds, rews, where = [], [], [], []
    for n, t0, t1 in _np_paths(dones, valid):
        f = _np_features(obs[:, t0:t1, n].T.astype(np.float64))
        feats.append(f)
        f = np.vstack([f, np.zeros(f.shape[1])])
        fds.append(f[1:] - f[:-1])
        rews.append(rewards[t0:t1, n].astype(np.float64))
        where += [(t, n) for t in range(t0, t1)]
    return np.concatenate(rews), np.vstack(feats), np.vstack(fds), where


def _np_dual(eta, v, rews, fd, eps, l2):
    """reps.py:102, :174-184 literally."""
    delta_v = rews + fd.dot(v)
    dual = eta * eps + eta * np.log(np.mean(np.exp(delta_v / eta - np.max(delta_v / eta)))) + \
        eta * np.max(delta_v / eta)
    return dual + l2 * (np.square(eta) + np.square(1 / eta))


def _np_dual_grad(eta, v, rews, fd, eps, l2):
    """Gradient of the expression above (what TT.grad of :187 evaluates), written out."""
    delta_v = rews + fd.dot(v)
    w = np.exp(delta_v / eta - np.max(delta_v / eta))
    d_eta = eps + np.log(np.mean(w)) + np.max(delta_v / eta) - (w * delta_v).sum() / (eta * w.sum()) + \
        l2 * (2 * eta - 2 / eta ** 3)
    return np.hstack([d_eta, (w[:, None] * fd).sum(axis=0) / w.sum()])


def _ragged_batch(seed, T=9, N=5, Do=3):
    """Column 0: a path ended by a done flag, then one ended by the last recorded step (two paths in a column).
    Column 1: a done flag, then an invalid tail.  Column 2: one path over all T steps, never done.  Column 3: done at the
    very last step.  Column 4: four short paths.  Observations outside +-10."""
    from rllab_amd.sampler.trajectories import Trajectories
    rng = np.random.RandomState(seed)
    obs = rng.randn(Do, T, N).astype(np.float32) * 3.0
    obs[0, 2, 0], obs[1, 5, 2], obs[2, 0, 4] = 37.5, -12.25, 10.5
    rewards = rng.randn(T, N).astype(np.float32)
    dones = np.zeros((T, N), np.uint8)
    valid = np.ones((T, N), bool)
    dones[3, 0] = 1
    dones[4, 1] = 1
    valid[5:, 1] = False
    dones[T - 1, 3] = 1
    dones[1, 4] = dones[2, 4] = dones[6, 4] = 1
    t = torch.as_tensor
    traj = Trajectories(t(obs), torch.zeros((1, T, N)), torch.zeros((1, T, N)), torch.zeros(1), t(rewards), t(dones), T)
    traj.valid = t(valid)
    traj.tin = traj.time_in_path().to(torch.int32)
    return traj, obs, rewards, dones, valid


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("seed,eta,l2", [(0, 15.0, 0.0), (1, 0.7, 1e-5), (2, 0.05, 0.0), (3, 300.0, 1e-3)])
def test_definition_matches_numpy_restatement(seed, eta, l2):
    from rllab_amd.algos import reps as R
    traj, obs, rewards, dones, valid = _ragged_batch(seed)
    rews, feats, fd, where = _np_batch(obs, rewards, dones, valid)
    assert len(_np_paths(dones, valid)) == 9 and len(where) == int(valid.sum())
    tt, nn = np.array(where).T
    phi = R.reps_features(traj.obs, traj.tin).numpy()
    fdt = R.reps_feat_diff(traj.obs, traj.tin, traj.dones, traj.valid).numpy()
    assert phi.dtype == np.float64 and phi.shape == (2 * 3 + 4,) + rewards.shape
    assert _rel(phi[:, tt, nn].T, feats) <= 1e-12
    assert _rel(fdt[:, tt, nn].T, fd) <= 1e-12
    assert np.abs(feats[:, :3]).max() == 10.0          # the clip is exercised
    eps = 0.5
    v = np.random.RandomState(seed + 10).randn(fd.shape[1])
    dual, grad = R.reps_dual(eta, v, traj.rewards, torch.as_tensor(fdt), traj.valid, eps, l2)
    want = _np_dual(eta, v, rews, fd, eps, l2)
    assert abs(dual - want) <= 1e-12 * abs(want)
    want_g = _np_dual_grad(eta, v, rews, fd, eps, l2)
    assert abs(grad[0] - want_g[0]) <= 1e-12 * max(1.0, np.abs(want_g).max())
    assert _rel(grad[1:], want_g[1:]) <= 1e-12
    w = R.reps_weights(eta, v, traj.rewards, torch.as_tensor(fdt), traj.valid).numpy()
    delta_v = rews + fd.dot(v)
    want_w = np.exp(delta_v / eta - np.max(delta_v / eta))
    assert np.abs(w[tt, nn] - want_w).max() <= 1e-12 and np.all(w[~valid] == 0) and w.max() == 1.0
    # analytic gradient against central finite differences of the dual
    x = np.hstack([eta, v])
    for i in range(len(x)):
        h = 1e-6 * max(1.0, abs(x[i]))
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        num = (_np_dual(xp[0], xp[1:], rews, fd, eps, l2) - _np_dual(xm[0], xm[1:], rews, fd, eps, l2)) / (2 * h)
        assert abs(num - grad[i]) <= 1e-5 * max(1.0, np.abs(grad).max()), (i, num, grad[i])


def test_dual_is_guarded_at_the_eta_bound():
    from rllab_amd.algos.reps import _positive_eta
    f = _positive_eta(lambda x: (1.0, np.ones(len(x))))
    val, g = f(np.array([0.0, 1.0, 2.0]))
    assert val == np.inf and np.all(g == 0) and f(np.array([1e-3, 1.0]))[0] == 1.0


def test_reps_iteration_on_cpu(quiet_logger):
    from rllab.algos.reps import REPS
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.misc import logger
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    from rllab_amd.sampler.base import SamplesData
    from rllab_amd.sampler.trajectories import PathList
    torch.manual_seed(0)
    np.random.seed(0)
    traj, obs, rewards, dones, valid = _ragged_batch(5, T=12, N=6)
    T, N = rewards.shape
    env = _Env(3, 2)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(8, 8))
    assert not pol.flat_params.is_cuda
    with torch.no_grad():
        means = pol.mean_planes(traj.obs.reshape(3, -1)).reshape(2, T, N)
    traj.means = means
    traj.actions = means + torch.randn(2, T, N)
    traj.act_dim = 2
    traj.log_std = pol.recorded_log_std()
    traj.advantages = torch.zeros(T, N)
    sd = SamplesData(_traj=traj, paths=PathList(traj))
    algo = REPS(env=env, policy=pol, baseline=ZeroBaseline(env.spec), sampler_cls=_NoSampler, max_opt_itr=20,
                L2_reg_dual=1e-5, L2_reg_loss=1e-4)
    algo.use_fused = False
    algo.init_opt()
    v0 = algo.param_v.copy()
    theta0 = pol.get_param_values()
    algo.optimize_policy(0, sd)
    tab = logger.get_tabular()
    keys = ["LossBefore", "LossAfter", "DualBefore", "DualAfter", "MeanKL"]
    assert all(k in tab for k in keys), sorted(tab)
    vals = {k: float(tab[k]) for k in keys}
    assert all(np.isfinite(x) for x in vals.values())
    assert algo.param_eta >= 0 and vals["DualAfter"] <= vals["DualBefore"] and vals["LossAfter"] <= vals["LossBefore"]
    assert vals["MeanKL"] > 0 and np.abs(pol.get_param_values() - theta0).max() > 0
    assert algo.param_eta != 15. and np.abs(algo.param_v - v0).max() > 0
    # the dual parameters are carried into the next call: it starts where this one ended
    dual_after = vals["DualAfter"]
    logger.dump_tabular()
    algo.optimize_policy(1, sd)
    tab = logger.get_tabular()
    assert abs(float(tab["DualBefore"]) - dual_after) <= 1e-9 * max(1.0, abs(dual_after))
    assert float(tab["DualAfter"]) <= float(tab["DualBefore"]) and algo.param_eta >= 0
    logger.dump_tabular()
    assert sorted(algo.get_itr_snapshot(1, sd)) == ["baseline", "env", "itr", "policy"]


def test_reps_refuses_env_shards(monkeypatch):
    from rllab.algos.reps import REPS
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    from rllab_amd.sampler import dist as D
    env = _Env(3, 2)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(8, 8))
    algo = REPS(env=env, policy=pol, baseline=ZeroBaseline(env.spec), sampler_cls=_NoSampler)
    monkeypatch.setattr(D, "is_distributed", lambda: True)
    with pytest.raises(NotImplementedError, match="shards"):
        algo.init_opt()


class _StubFused(object):
    """Records which objective an optimizer asks for."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def accepts(self, inputs):
        return True

    def value_and_grad(self, inputs, penalty=0.0, vpg=False):
        self.calls.append(("value_and_grad", bool(vpg)))
        return 1.0, np.zeros(self.n)

    def loglik_loss(self, inputs):
        self.calls.append(("loglik_loss",))
        return 2.0

    def loss_and_kl(self, inputs):
        self.calls.append(("loss_and_kl",))
        return 3.0, 0.0

    def loss_stats_host(self, inputs):
        return (0.0, 0.0, 0.0, 0.0)

    def release(self):
        pass


@pytest.mark.parametrize("name", ["vpg", "erwr"])
def test_lbfgs_is_told_to_use_the_log_likelihood_objective(name, quiet_logger):
    from rllab.algos.erwr import ERWR
    from rllab.algos.vpg import VPG
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.optimizers.lbfgs_optimizer import LbfgsOptimizer
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    env = _Env(3, 2)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(8, 8))
    stub = _StubFused(len(pol.get_param_values(trainable=True)))
    pol.fused_ops = lambda: stub
    kw = dict(env=env, policy=pol, baseline=ZeroBaseline(env.spec), sampler_cls=_NoSampler)
    algo = ERWR(**kw) if name == "erwr" else VPG(optimizer=LbfgsOptimizer(max_opt_itr=2), **kw)
    algo.init_opt()
    inputs = (torch.zeros(3, 4),)
    assert algo.optimizer.loss(inputs) == 2.0
    algo.optimizer.optimize(inputs)
    assert ("loglik_loss",) in stub.calls and ("value_and_grad", True) in stub.calls
    assert ("loss_and_kl",) not in stub.calls and ("value_and_grad", False) not in stub.calls


def test_lbfgs_built_as_the_regressor_builds_it_asks_as_before():
    from rllab_amd.optimizers.lbfgs_optimizer import LbfgsOptimizer
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    pol = GaussianMLPPolicy(_spec(3, 2), hidden_sizes=(8, 8))
    stub = _StubFused(len(pol.get_param_values(trainable=True)))
    opt = LbfgsOptimizer(max_opt_itr=2)
    # regressors/gaussian_mlp_regressor.py: update_opt(loss=, target=, inputs=None, fused=)
    opt.update_opt(loss=lambda flat, x: (flat ** 2).sum(), target=pol, inputs=None, fused=stub)
    inputs = (torch.zeros(3, 4),)
    assert opt.loss(inputs) == 3.0
    opt.optimize(inputs)
    assert ("loss_and_kl",) in stub.calls and ("value_and_grad", False) in stub.calls
    assert ("loglik_loss",) not in stub.calls and ("value_and_grad", True) not in stub.calls
