#!/usr/bin/env python
"""Train the cross-entropy method on Cartpole with a recurrent policy (GaussianGRUPolicy).

Every iteration draws a population of parameter vectors around the current mean -- h0, the GRU's weights and log_std --,
evaluates ALL of them in one launch of the recurrent population rollout (one candidate per env, every lane its own GRU:
rl_rollout_population_gru) and refits mean and std to the best 5 %.  No back-propagation through time anywhere: the whole
loop runs on kernels.

  python examples/cem_gru_cartpole.py
  python examples/cem_gru_cartpole.py --n-samples 4096 --n-itr 30 --csv cem_gru.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.cem import CEM  # noqa: E402
from rllab.envs.box2d.cartpole_env import CartpoleEnv  # noqa: E402
from rllab.envs.normalized_env import normalize  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.policies.gaussian_gru_policy import GaussianGRUPolicy  # noqa: E402

# tools/exp/cem_gru_cpu_curves.py (the CPU yardstick) and tests/test_gpu_population_gru.py run this very configuration
CONFIG = dict(hidden_sizes=(32,), n_itr=20, n_samples=100, n_evals=1, max_path_length=100, discount=0.99, init_std=1.0,
              extra_std=1.0, extra_decay_time=100, best_frac=0.05)


def make_algo(seed=1, **overrides):
    """CEM on normalize(CartpoleEnv()) with a GaussianGRUPolicy under ``CONFIG``; ``overrides``: CEM arguments."""
    ext.set_seed(seed)
    env = normalize(CartpoleEnv())
    policy = GaussianGRUPolicy(env_spec=env.spec, hidden_sizes=CONFIG["hidden_sizes"])
    kw = {k: v for k, v in CONFIG.items() if k != "hidden_sizes"}
    kw.update(overrides)
    return CEM(env=env, policy=policy, seed=seed, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-samples", type=int, default=CONFIG["n_samples"])
    ap.add_argument("--n-evals", type=int, default=CONFIG["n_evals"])
    ap.add_argument("--n-itr", type=int, default=CONFIG["n_itr"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--csv", default=None, help="write the tabular log (one row per iteration) to this file")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    if args.csv:
        logger.add_tabular_output(args.csv)
    if args.quiet:
        logger.set_quiet(True)
    make_algo(args.seed, n_itr=args.n_itr, n_samples=args.n_samples, n_evals=args.n_evals).train()


if __name__ == "__main__":
    main()
