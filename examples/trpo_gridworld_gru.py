#!/usr/bin/env python
"""Train TRPO on GridWorld with a recurrent policy (CategoricalGRUPolicy) on the lock-step GPU sampler.

Sampling is one kernel launch per batch: every env steps its GRU, draws its action and moves on the map for the whole
horizon (rl_rollout_gridworld_gru).  The update -- loss, gradient, finite-difference Hessian-vector products -- runs
through torch autograd as a scan over the time axis of the dense batch planes.  With --bptt-kernels it runs on the HIP
kernels (rl_gru_categorical_eval / _grad / _fvp), the products being Fisher-vector products.

  python examples/trpo_gridworld_gru.py
  python examples/trpo_gridworld_gru.py --bptt-kernels
  python examples/trpo_gridworld_gru.py --n-itr 20 --csv gridworld_gru.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.trpo import TRPO  # noqa: E402
from rllab.baselines.linear_feature_baseline import LinearFeatureBaseline  # noqa: E402
from rllab.envs.grid_world_env import GridWorldEnv  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, FiniteDifferenceHvp  # noqa: E402
from rllab.policies.categorical_gru_policy import CategoricalGRUPolicy  # noqa: E402

# tools/exp/trpo_gridworld_gru_cpu.py (the CPU yardstick) and tests/test_gpu_categorical_gru.py run this very configuration
CONFIG = dict(desc="4x4", batch_size=2000, max_path_length=20, n_itr=10, discount=0.99, step_size=0.01,
              hvp_base_eps=1e-5)


def make_algo(seed=1, n_itr=None, bptt_kernels=False):
    ext.set_seed(seed)
    env = GridWorldEnv(CONFIG["desc"])
    policy = CategoricalGRUPolicy(env_spec=env.spec, bptt_kernels=bptt_kernels)
    baseline = LinearFeatureBaseline(env_spec=env.spec)
    # on the recurrent kernels the optimizer's default products are the Fisher-vector kernel
    optimizer = ConjugateGradientOptimizer() if bptt_kernels else \
        ConjugateGradientOptimizer(hvp_approach=FiniteDifferenceHvp(base_eps=CONFIG["hvp_base_eps"]))
    return TRPO(env=env, policy=policy, baseline=baseline, batch_size=CONFIG["batch_size"],
                max_path_length=CONFIG["max_path_length"], n_itr=CONFIG["n_itr"] if n_itr is None else n_itr,
                discount=CONFIG["discount"], step_size=CONFIG["step_size"], optimizer=optimizer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-itr", type=int, default=CONFIG["n_itr"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--csv", default=None, help="write the tabular log (one row per iteration) to this file")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--bptt-kernels", action="store_true",
                    help="run the update on the recurrent HIP kernels (CategoricalGRUPolicy(bptt_kernels=True))")
    args = ap.parse_args()
    if args.csv:
        logger.add_tabular_output(args.csv)
    if args.quiet:
        logger.set_quiet(True)
    make_algo(args.seed, args.n_itr, bptt_kernels=args.bptt_kernels).train()


if __name__ == "__main__":
    main()
