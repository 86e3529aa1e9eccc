"""DDPG(rollout_steps=S): collection and evaluation in the fused deterministic rollout -- the schedule of launches, the
pool rows a chunk writes, and the example script."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_ddpg import EVAL_KEYS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def tabular(quiet_logger, tmp_path):
    """The rows ``logger.dump_tabular`` writes during the test, as a list of dicts (read after training)."""
    from rllab_amd.misc import logger
    path = str(tmp_path / "progress.csv")
    logger.add_tabular_output(path)
    yield lambda: list(csv.DictReader(open(path)))
    logger.remove_tabular_output(path)


def _train_counted(monkeypatch, rollout_steps):
    from rllab_amd import _lib
    from rllab_amd.envs.hip_env import HipVecEnv
    from rllab.algos.ddpg import DDPG
    from rllab.envs.box2d.cartpole_env import CartpoleEnv
    from rllab.exploration_strategies.ou_strategy import OUStrategy
    from rllab.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    updates, rollouts = [], []
    real_update, real_rollout = _lib.lib.rl_ddpg_update, _lib.lib.rl_rollout_deterministic_mlp

    def counted_update(args, stream):
        updates.append(args._obj.n_updates)            # args: ctypes.byref of the launch's argument block
        return real_update(args, stream)

    def counted_rollout(args, stream):
        rollouts.append((args._obj.explore, args._obj.horizon, args._obj.reset_at_start))
        return real_rollout(args, stream)

    def no_step(self, *a, **kw):
        raise AssertionError("HipVecEnv.step called under rollout_steps")

    monkeypatch.setattr(_lib.lib, "rl_ddpg_update", counted_update)
    monkeypatch.setattr(_lib.lib, "rl_rollout_deterministic_mlp", counted_rollout)
    monkeypatch.setattr(HipVecEnv, "step", no_step)
    env = CartpoleEnv()
    policy, qf, es = DeterministicMLPPolicy(env.spec), ContinuousMLPQFunction(env.spec), OUStrategy(env.spec)
    algo = DDPG(env=env, policy=policy, qf=qf, es=es, n_epochs=1, epoch_length=100, batch_size=32, min_pool_size=50,
                replay_pool_size=1000, eval_samples=100, n_envs=8, rollout_steps=rollout_steps)
    algo.train()
    return algo, es, updates, rollouts


def test_schedule_of_a_chunked_epoch(tabular, monkeypatch):
    """ceil(100 / 8) = 13 lock-steps in launches of 4, 4, 4, 1; the pool holds 32, 64, 96, 104 rows behind them and
    reaches 50 with the second lock-step of the second launch: 0, 2, 4 and 1 lock-steps' worth of 8 updates."""
    from rllab_amd import _lib
    algo, es, updates, rollouts = _train_counted(monkeypatch, 4)
    assert updates == [16, 32, 8]
    assert algo.pool.size == 104 and algo.itr == 104
    assert algo.opt_info["update"].step_counts() == (56, 56)
    assert es.states.shape == (8, 1)
    collection = [r for r in rollouts if r[0] != _lib.EXPLORE_NONE]
    assert collection == [(_lib.EXPLORE_OU, 4, 1), (_lib.EXPLORE_OU, 4, 0), (_lib.EXPLORE_OU, 4, 0), (_lib.EXPLORE_OU, 1, 0)]
    evaluation = [r for r in rollouts if r[0] == _lib.EXPLORE_NONE]
    assert len(evaluation) >= 1 and evaluation[0][2] == 1 and all(r[2] == 0 for r in evaluation[1:])
    assert "fused deterministic rollout" in algo.eval_sampler.sampling_path(algo.policy)[0]
    rows = tabular()
    assert len(rows) == 1
    for k in EVAL_KEYS + ["AverageEsReturn", "StdEsReturn", "MaxEsReturn", "MinEsReturn"]:
        assert k in rows[0] and np.isfinite(float(rows[0][k])), k
    for obj in (algo.policy, algo.qf, algo.opt_info["target_policy"], algo.opt_info["target_qf"]):
        assert np.all(np.isfinite(obj.get_param_values()))


def test_one_lock_step_per_launch_is_the_loops_schedule(tabular, monkeypatch):
    algo, es, updates, rollouts = _train_counted(monkeypatch, 1)
    assert updates == [8] * 7
    assert algo.pool.size == 104 and algo.itr == 104 and algo.opt_info["update"].step_counts() == (56, 56)
    assert [r[1] for r in rollouts if r[0] != 0] == [1] * 13


@pytest.mark.parametrize("include", [False, True])
def test_pool_rows_of_chunks(include, quiet_logger):
    """normalize(CartpoleEnv()), scale_reward = 0.01, paths cut at 30 steps, launches of 5 lock-steps: the pool's rows
    are the launches' planes, t-major -- term = dones, skip = cuts unless include_horizon_terminal_transitions,
    rew = rewards * scale_reward, obs the observation plane and next_obs the plane one lock-step later wherever the
    path went on."""
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
    # An untrained policy drops the pole within ten steps: no path would reach the horizon.  This one leans against the
    # pole, a = tanh(-(5 angle + angular velocity)) through two rectify units per layer, and the noise tips some paths
    # over all the same: the host env under numpy draws ends 11 .. 21 paths and cuts 7 .. 12 in 600 steps.
    flat = np.zeros_like(policy.get_param_values())
    w0, w1, w2 = flat[:4 * 32].reshape(4, 32), flat[4 * 32 + 32:4 * 32 + 32 + 32 * 32].reshape(32, 32), flat[-33:-1]
    w0[2, 0], w0[3, 0], w0[2, 1], w0[3, 1] = 5.0, 1.0, -5.0, -1.0
    w1[0, 0] = w1[1, 1] = 1.0
    w2[0], w2[1] = -1.0, 1.0
    policy.set_param_values(flat)
    es = OUStrategy(env.spec, sigma=0.3)
    n, horizon, steps = 4, 30, 150
    seen = []

    class Recording(DDPG):
        def start_worker(self):
            DDPG.start_worker(self)
            launch = self.vec_env.rollout_deterministic

            def recorded(*a, **kw):
                traj = launch(*a, **kw)
                seen.append(traj)
                return traj
            self.vec_env.rollout_deterministic = recorded

    algo = Recording(env=env, policy=policy, qf=qf, es=es, n_epochs=1, epoch_length=n * steps, batch_size=32,
                     min_pool_size=64, replay_pool_size=1000, eval_samples=100, max_path_length=horizon,
                     scale_reward=0.01, include_horizon_terminal_transitions=include, n_envs=n, rollout_steps=5,
                     policy_learning_rate=1e-5)
    algo.train()
    assert len(seen) == steps // 5 and all(t.T == 5 for t in seen)
    assert algo.pool.size == n * steps and algo.pool.top == n * steps
    cat = lambda name, dim: torch.cat([getattr(t, name) for t in seen], dim=dim).cpu().numpy()
    done, cuts, rew, obs = cat("dones", 0).astype(bool), cat("cuts", 0).astype(bool), cat("rewards", 0), cat("obs", 1)
    length = np.zeros(n, dtype=np.int64)
    for t in range(steps):                                    # a cut is a path's 30th step, and the env had not ended it
        length += 1
        assert np.all(length[cuts[t]] == horizon) and np.all(done[t][length >= horizon])
        length[done[t]] = 0
    print("paths ended by the env: %d, cut at the horizon: %d" % ((done & ~cuts).sum(), cuts.sum()))
    assert (done & ~cuts).sum() > 0 and cuts.sum() > 0
    pool = algo.pool
    rows = lambda x: x[:n * steps].cpu().numpy().reshape(steps, n, -1)
    assert np.array_equal(rows(pool.term)[..., 0], done.astype(np.float32))
    want_skip = np.zeros_like(cuts) if include else cuts
    assert np.array_equal(rows(pool.skip)[..., 0], want_skip.astype(np.float32))
    assert np.array_equal(rows(pool.rew)[..., 0], rew * np.float32(0.01))
    assert np.array_equal(rows(pool.obs), obs.transpose(1, 2, 0))
    assert np.array_equal(rows(pool.act), cat("actions", 1).transpose(1, 2, 0))
    nxt = rows(pool.next_obs)
    went_on = ~done[:-1]
    assert went_on.sum() > 0 and np.array_equal(nxt[:-1][went_on], obs.transpose(1, 2, 0)[1:][went_on])
    if not done[-1].all():                                    # the last row: the observation the executor carries
        carried = algo.vec_env._obs.t().cpu().numpy()
        assert np.array_equal(nxt[-1][~done[-1]], carried[~done[-1]])


def test_example_script_runs_with_rollout_steps():
    """examples/ddpg_cartpole.py --rollout-steps 10 in a fresh child process."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ddpg_cartpole.py"), "--n-epochs", "1",
                          "--epoch-length", "200", "--n-envs", "4", "--min-pool-size", "100", "--rollout-steps", "10"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0, out.stdout.decode()[-2000:]
    assert b"fused deterministic rollout" in out.stdout
