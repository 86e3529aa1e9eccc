#!/usr/bin/env python
"""Time per lock-step of DDPG's collection on an MI355X (needs the GPU): the per-transition loop against the fused
deterministic rollout.

normalize(CartpoleEnv()), (32, 32) policy, OUStrategy, paths cut at 100 steps, no updates (the pool never reaches
``min_pool_size``: what is timed is collection alone -- actions, env steps, resets, the pool write and the path
returns).  Per ``n_envs`` in 1, 64, 4096 the median of 7 measurements, each 100 lock-steps between two host clock reads
with the device drained at both, of

* the loop of ``DDPG.train`` with ``rollout_steps=None`` -- restated here line by line, because ``train`` does not
  hand out its inner loop;
* ``DDPG._collect_fused`` at ``rollout_steps`` 1, 10 and 100 (``rollout_steps`` is set on the object behind the
  constructor: with updates, 4096 envs x 100 lock-steps would be more updates than one launch of the update kernel
  runs, and DDPG refuses it).

  python tools/ddpg_rollout_time.py --out profiles/ddpg_rollout_time.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_ENVS = (1, 64, 4096)
ROLLOUT_STEPS = (1, 10, 100)
LOCK_STEPS = 100
MAX_PATH_LENGTH = 100


def wall_us_per_step(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / LOCK_STEPS


def make(n_envs, rollout_steps):
    from rllab_amd.algos.ddpg import DDPG
    from rllab_amd.algos.replay_pool import DeviceReplayPool
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.exploration_strategies.ou_strategy import OUStrategy
    from rllab_amd.misc import ext
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab_amd.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    ext.set_seed(1)
    env = normalize(CartpoleEnv())
    algo = DDPG(env=env, policy=DeterministicMLPPolicy(env.spec, hidden_sizes=(32, 32)),
                qf=ContinuousMLPQFunction(env.spec, hidden_sizes=(32, 32)), es=OUStrategy(env.spec), batch_size=32,
                epoch_length=LOCK_STEPS * n_envs, min_pool_size=2 ** 40, replay_pool_size=1000000,
                max_path_length=MAX_PATH_LENGTH, scale_reward=0.01, n_envs=n_envs,
                rollout_steps=None if rollout_steps is None else 1)
    algo.rollout_steps = rollout_steps
    algo.pool = DeviceReplayPool(algo.replay_pool_size, env.observation_space.flat_dim, env.action_space.flat_dim)
    algo.start_worker()
    algo.init_opt()
    algo.itr = 0
    algo._es_returns = torch.full((LOCK_STEPS, n_envs), float("nan"), dtype=torch.float64, device=algo.pool.device)
    algo.es.reset()
    return algo


def loop_epochs(algo):
    """The collection of ``DDPG.train`` with ``rollout_steps=None`` (algos/ddpg.py), an epoch per call."""
    vec, n, pool, dev = algo.vec_env, algo.n_envs, algo.pool, algo.pool.device
    st = dict(path_length=torch.zeros(n, dtype=torch.int64, device=dev),
              path_return=torch.zeros(n, dtype=torch.float64, device=dev), observation=vec.reset().clone())

    def epoch():
        path_length, path_return, observation = st["path_length"], st["path_return"], st["observation"]
        for epoch_itr in range(LOCK_STEPS):
            action = algo.es.get_actions(algo.itr, observation, policy=algo.policy)
            next_observation, reward, done, _ = vec.step(action)
            path_length += 1
            path_return += reward.to(torch.float64)
            horizon = (~done) & (path_length >= algo.max_path_length)
            terminal = done | horizon
            pool.add(observation, action, reward * algo.scale_reward, terminal, next_observation,
                     horizon.to(torch.float32))
            observation = vec.reset(mask=horizon).clone()
            algo.es.reset(mask=terminal)
            algo._es_returns[epoch_itr] = torch.where(terminal, path_return, algo._es_returns[epoch_itr])
            path_length.masked_fill_(terminal, 0)
            path_return.masked_fill_(terminal, 0.0)
            algo.itr += n
        st["observation"] = observation
    return epoch


def fused_epochs(algo):
    path_return = torch.zeros(algo.n_envs, dtype=torch.float64, device=algo.pool.device)
    first = [True]

    def epoch():
        algo._collect_fused(LOCK_STEPS, path_return, first=first[0])
        first[0] = False
    return epoch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run cannot give a time"
    from rllab_amd.misc import logger
    logger.set_quiet(True)
    results = []
    for n in N_ENVS:
        row = dict(n_envs=n, lock_steps=LOCK_STEPS, hidden=[32, 32], env="normalize(CartpoleEnv())")
        for S in (None,) + ROLLOUT_STEPS:
            algo = make(n, S)
            epoch = loop_epochs(algo) if S is None else fused_epochs(algo)
            epoch()                                              # warm-up
            us = float(np.median([wall_us_per_step(epoch) for _ in range(7)]))
            row["loop_us_per_lock_step" if S is None else "fused_us_per_lock_step_S%d" % S] = round(us, 2)
            assert algo.pool.size == min(8 * LOCK_STEPS * n, algo.pool.capacity)
        print(json.dumps(row))
        results.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), median_of=7, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
