#!/usr/bin/env python
"""Train TRPO on GridWorld with a categorical MLP policy: discrete actions on the lock-step GPU sampler.

Observations are one-hot, so the rollout samples from the policy's probability table -- every env's whole horizon in one
kernel launch; loss, gradient and Fisher-vector products of the update run on the categorical head kernels.

  python examples/trpo_gridworld.py
  python examples/trpo_gridworld.py --map 4x4_safe --n-envs 256 --n-itr 30 --csv gridworld.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.trpo import TRPO  # noqa: E402
from rllab.baselines.linear_feature_baseline import LinearFeatureBaseline  # noqa: E402
from rllab.envs.grid_world_env import GridWorldEnv  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.policies.categorical_mlp_policy import CategoricalMLPPolicy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="4x4", help="chain, 4x4_safe, 4x4 or 8x8")
    ap.add_argument("--n-envs", type=int, default=80)
    ap.add_argument("--n-itr", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--csv", default=None, help="write the tabular log (one row per iteration) to this file")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    if args.csv:
        logger.add_tabular_output(args.csv)
    if args.quiet:
        logger.set_quiet(True)
    ext.set_seed(args.seed)
    env = GridWorldEnv(args.map)
    policy = CategoricalMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    baseline = LinearFeatureBaseline(env_spec=env.spec)
    algo = TRPO(env=env, policy=policy, baseline=baseline, batch_size=args.n_envs * 50, max_path_length=50,
                n_itr=args.n_itr, discount=0.99, step_size=0.01, sampler_args=dict(n_envs=args.n_envs))
    algo.train()


if __name__ == "__main__":
    main()
