#!/usr/bin/env python
"""Train the cross-entropy method on Cartpole: the set-up of the reference's examples/trpo_cartpole.py with CEM.

Every iteration draws a population of parameter vectors around the current mean, evaluates ALL of them in one launch
of the population rollout (one candidate per env, rl_rollout_population) and refits mean and std to the best 5 %.

  python examples/cem_cartpole.py
  python examples/cem_cartpole.py --n-samples 4096 --n-itr 30 --csv cem.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.cem import CEM  # noqa: E402
from rllab.envs.box2d.cartpole_env import CartpoleEnv  # noqa: E402
from rllab.envs.normalized_env import normalize  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.policies.gaussian_mlp_policy import GaussianMLPPolicy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-samples", type=int, default=100)
    ap.add_argument("--n-evals", type=int, default=1)
    ap.add_argument("--n-itr", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--csv", default=None, help="write the tabular log (one row per iteration) to this file")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    if args.csv:
        logger.add_tabular_output(args.csv)
    if args.quiet:
        logger.set_quiet(True)
    ext.set_seed(args.seed)
    env = normalize(CartpoleEnv())
    # The neural network policy should have two hidden layers, each with 32 hidden units.
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    algo = CEM(env=env, policy=policy, n_itr=args.n_itr, n_samples=args.n_samples, n_evals=args.n_evals,
               max_path_length=100, discount=0.99)
    algo.train()


if __name__ == "__main__":
    main()
