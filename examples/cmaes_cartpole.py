#!/usr/bin/env python
"""Train CMA-ES on Cartpole: the set-up of the reference's examples/trpo_cartpole.py with rllab.algos.cma_es.CMAES.

Every iteration asks the search distribution (mean, step size sigma, full covariance C, all on the device in float64) for
a population of parameter vectors, evaluates ALL of them in one launch of the population rollout (one candidate per env,
rl_rollout_population) and tells the distribution their fitness; the N x N update of C is one HIP kernel
(rl_cmaes_cov_update).

  python examples/cmaes_cartpole.py
  python examples/cmaes_cartpole.py --popsize 256 --n-itr 30 --csv cmaes.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.cma_es import CMAES  # noqa: E402
from rllab.envs.box2d.cartpole_env import CartpoleEnv  # noqa: E402
from rllab.envs.normalized_env import normalize  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.policies.gaussian_mlp_policy import GaussianMLPPolicy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--popsize", type=int, default=None, help="default: 4 + int(3 ln N)")
    ap.add_argument("--batch-size", type=int, default=None, help="samples per iteration instead of a fixed population")
    ap.add_argument("--sigma0", type=float, default=1.0)
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
    algo = CMAES(env=env, policy=policy, n_itr=args.n_itr, sigma0=args.sigma0, batch_size=args.batch_size,
                 popsize=args.popsize, max_path_length=100, discount=0.99)
    algo.train()
    print("final sigma %.4g, %d eigendecompositions, stop: %r" % (float(algo.es.sigma), algo.es.count_eigen,
                                                                   algo.stop_dict or None))


if __name__ == "__main__":
    main()
