"""DDPG end to end on the device: the reference's ``test_ddpg`` (tests/test_algos.py:97-111) through the ``rllab``
alias, the lock-step variant, one launch of the update per lock-step, the replay pool's skip rule, the example script
and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_KEYS = ["Epoch", "AverageReturn", "StdReturn", "MaxReturn", "MinReturn", "AverageDiscountedReturn", "AverageQLoss",
             "AveragePolicySurr", "AverageQ", "AverageAbsQ", "AverageY", "AverageAbsY", "AverageAbsQYDiff",
             "AverageAction", "PolicyRegParamNorm", "QFunRegParamNorm"]


@pytest.fixture
def tabular(quiet_logger, tmp_path):
    """The rows ``logger.dump_tabular`` writes during the test, as a list of dicts (read after training)."""
    import csv
    from rllab_amd.misc import logger
    path = str(tmp_path / "progress.csv")
    logger.add_tabular_output(path)
    yield lambda: list(csv.DictReader(open(path)))
    logger.remove_tabular_output(path)


def _check_trained(algo, rows):
    assert len(rows) == 1
    for k in EVAL_KEYS:
        assert k in rows[0] and np.isfinite(float(rows[0][k])), k
    for obj in (algo.policy, algo.qf, algo.opt_info["target_policy"], algo.opt_info["target_qf"]):
        assert np.all(np.isfinite(obj.get_param_values()))
    snap = algo.get_epoch_snapshot(0)
    assert sorted(snap) == ["env", "epoch", "es", "policy", "qf", "target_policy", "target_qf"]


def test_ddpg(tabular):
    from rllab.algos.ddpg import DDPG
    from rllab.envs.box2d.cartpole_env import CartpoleEnv
    from rllab.exploration_strategies.ou_strategy import OUStrategy
    from rllab.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    env = CartpoleEnv()
    policy = DeterministicMLPPolicy(env.spec)
    qf = ContinuousMLPQFunction(env.spec)
    es = OUStrategy(env.spec)
    before = policy.get_param_values()
    algo = DDPG(
        env=env, policy=policy, qf=qf, es=es,
        n_epochs=1,
        epoch_length=100,
        batch_size=32,
        min_pool_size=50,
        replay_pool_size=1000,
        eval_samples=100,
    )
    algo.train()
    assert not np.any(np.isnan(policy.get_param_values()))
    _check_trained(algo, tabular())
    assert algo.pool.size == 100 and algo.itr == 100
    assert algo.opt_info["update"].step_counts() == (51, 51)         # updates begin once the pool holds 50 rows
    assert np.abs(policy.get_param_values() - before).max() > 0
    # the targets trail the parameters (tau = 1e-3): they moved, and less than the parameters did
    tp, p = algo.opt_info["target_policy"].get_param_values(), policy.get_param_values()
    assert 0 < np.abs(tp - before).max() < np.abs(p - before).max()


def test_ddpg_eight_envs_one_launch_per_lock_step(tabular, monkeypatch):
    from rllab_amd import _lib
    from rllab.algos.ddpg import DDPG
    from rllab.envs.box2d.cartpole_env import CartpoleEnv
    from rllab.exploration_strategies.ou_strategy import OUStrategy
    from rllab.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    calls = []
    real = _lib.lib.rl_ddpg_update

    def counted(args, stream):
        calls.append(args._obj.n_updates)            # args: ctypes.byref of the launch's rl_ddpg_args
        return real(args, stream)

    monkeypatch.setattr(_lib.lib, "rl_ddpg_update", counted)
    env = CartpoleEnv()
    policy, qf, es = DeterministicMLPPolicy(env.spec), ContinuousMLPQFunction(env.spec), OUStrategy(env.spec)
    algo = DDPG(env=env, policy=policy, qf=qf, es=es, n_epochs=1, epoch_length=100, batch_size=32, min_pool_size=50,
                replay_pool_size=1000, eval_samples=100, n_envs=8)
    algo.train()
    _check_trained(algo, tabular())
    # ceil(100 / 8) = 13 lock-steps of 8 transitions; the pool reaches 50 rows with the 7th: 7 launches of 8 updates
    assert algo.pool.size == 104 and algo.itr == 104
    assert calls == [8] * 7
    assert algo.opt_info["update"].step_counts() == (56, 56)
    assert es.states.shape == (8, 1)


@pytest.mark.parametrize("include", [False, True])
def test_pool_rows_follow_the_skip_rule(include, quiet_logger):
    """normalize(CartpoleEnv()), scale_reward = 0.01, paths cut at 30 steps: a pool row has term = 1 where its path ended
    for either reason, and skip = 1 exactly where the path was cut at the horizon, the env had not terminated and
    include_horizon_terminal_transitions is off -- recounted here from the env's own done flags."""
    from rllab.algos.ddpg import DDPG
    from rllab.envs.box2d.cartpole_env import CartpoleEnv
    from rllab.envs.normalized_env import normalize
    from rllab.exploration_strategies.ou_strategy import OUStrategy
    from rllab.misc import ext
    from rllab.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    ext.set_seed(3)
    env = normalize(CartpoleEnv())
    policy, qf = DeterministicMLPPolicy(env.spec), ContinuousMLPQFunction(env.spec)
    es = OUStrategy(env.spec, sigma=1.0)                      # strong noise: some paths end before the horizon
    n, horizon, steps = 4, 30, 150
    seen = []

    class Recording(DDPG):
        def start_worker(self):
            DDPG.start_worker(self)
            step = self.vec_env.step

            def recorded(action):
                out = step(action)
                seen.append((out[1].clone(), out[2].clone()))
                return out
            self.vec_env.step = recorded

    algo = Recording(env=env, policy=policy, qf=qf, es=es, n_epochs=1, epoch_length=n * steps, batch_size=32,
                     min_pool_size=64, replay_pool_size=1000, eval_samples=100, max_path_length=horizon,
                     scale_reward=0.01, include_horizon_terminal_transitions=include, n_envs=n)
    algo.train()
    assert len(seen) == steps and algo.pool.size == n * steps and algo.pool.top == n * steps
    done = torch.stack([d for _, d in seen]).cpu().numpy()            # [steps, n]
    rew = torch.stack([r for r, _ in seen]).cpu().numpy()
    length = np.zeros(n, dtype=np.int64)
    term = np.zeros((steps, n), dtype=bool)
    cut = np.zeros((steps, n), dtype=bool)
    for t in range(steps):
        length += 1
        cut[t] = ~done[t] & (length >= horizon)
        term[t] = done[t] | cut[t]
        length[term[t]] = 0
    print("paths ended by the env: %d, cut at the horizon: %d" % (done.sum(), cut.sum()))
    assert done.sum() > 0 and cut.sum() > 0
    pool = algo.pool
    assert np.array_equal(pool.term[:n * steps].cpu().numpy().reshape(steps, n), term.astype(np.float32))
    want_skip = np.zeros_like(cut) if include else cut
    assert np.array_equal(pool.skip[:n * steps].cpu().numpy().reshape(steps, n), want_skip.astype(np.float32))
    assert np.allclose(pool.rew[:n * steps].cpu().numpy().reshape(steps, n), 0.01 * rew, rtol=1e-6, atol=0)


def test_example_script_runs():
    """examples/ddpg_cartpole.py in a fresh child process (the script has its own min_pool_size of 10 000: nothing is
    updated in 200 steps, the control flow around it runs)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ddpg_cartpole.py"), "--n-epochs", "1",
                          "--epoch-length", "200"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0, out.stdout.decode()[-2000:]


def test_refusals():
    from rllab.algos.ddpg import DDPG
    from rllab.envs.box2d.cartpole_env import CartpoleEnv
    from rllab.exploration_strategies.ou_strategy import OUStrategy
    from rllab.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    env = CartpoleEnv()
    es = OUStrategy(env.spec)
    with pytest.raises(NotImplementedError, match="at most 64 units"):
        DDPG(env=env, policy=DeterministicMLPPolicy(env.spec, hidden_sizes=(128, 128)),
             qf=ContinuousMLPQFunction(env.spec, hidden_sizes=(128, 128)), es=es)
    with pytest.raises(NotImplementedError, match="two hidden layers"):
        DDPG(env=env, policy=DeterministicMLPPolicy(env.spec, hidden_sizes=(32, 32, 32)),
             qf=ContinuousMLPQFunction(env.spec, hidden_sizes=(32, 32, 32)), es=es)
    with pytest.raises(NotImplementedError, match="batch normalisation"):
        DeterministicMLPPolicy(env.spec, bn=True)
    with pytest.raises(NotImplementedError, match="batch normalisation"):
        ContinuousMLPQFunction(env.spec, bn=True)
    with pytest.raises(NotImplementedError, match="1 .. 128"):
        DDPG(env=env, policy=DeterministicMLPPolicy(env.spec), qf=ContinuousMLPQFunction(env.spec), es=es, batch_size=256)
    with pytest.raises(NotImplementedError, match="1 .. 16384"):
        DDPG(env=env, policy=DeterministicMLPPolicy(env.spec), qf=ContinuousMLPQFunction(env.spec), es=es, n_envs=4096,
             n_updates_per_sample=8)
