#!/usr/bin/env python
"""Train ERWR (episodic reward-weighted regression) on Cartpole with the lock-step GPU sampler.

The policy is fitted by L-BFGS to -mean(log p(a|o) * adv) with the advantages shifted to be positive; every
evaluation of value and gradient is one kernel launch over the batch.

  python examples/erwr_cartpole.py
  python examples/erwr_cartpole.py --n-envs 4096 --n-itr 30 --csv erwr.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.erwr import ERWR  # noqa: E402
from rllab.baselines.linear_feature_baseline import LinearFeatureBaseline  # noqa: E402
from rllab.envs.box2d.cartpole_env import CartpoleEnv  # noqa: E402
from rllab.envs.normalized_env import normalize  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.policies.gaussian_mlp_policy import GaussianMLPPolicy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1024)
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
    env = normalize(CartpoleEnv())
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    baseline = LinearFeatureBaseline(env_spec=env.spec)
    algo = ERWR(env=env, policy=policy, baseline=baseline, batch_size=args.n_envs * 100, max_path_length=100,
                n_itr=args.n_itr, discount=0.99, sampler_args=dict(n_envs=args.n_envs))
    algo.train()


if __name__ == "__main__":
    main()
