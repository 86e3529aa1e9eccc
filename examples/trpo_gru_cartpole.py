#!/usr/bin/env python
"""Train TRPO on Cartpole with a recurrent policy (GaussianGRUPolicy) on the lock-step GPU sampler.

Sampling is one kernel launch per batch: every env steps its GRU and its dynamics for the whole horizon
(rl_rollout_gaussian_gru).  The update -- loss, gradient, finite-difference Hessian-vector products -- runs through torch
autograd as a scan over the time axis of the dense batch planes; with --bptt-kernels it runs on the recurrent update
kernels (rl_gru_gaussian_eval / _grad / _fvp), the products being Fisher-vector products.

  python examples/trpo_gru_cartpole.py
  python examples/trpo_gru_cartpole.py --bptt-kernels
  python examples/trpo_gru_cartpole.py --n-itr 20 --csv gru_cartpole.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.trpo import TRPO  # noqa: E402
from rllab.baselines.linear_feature_baseline import LinearFeatureBaseline  # noqa: E402
from rllab.envs.box2d.cartpole_env import CartpoleEnv  # noqa: E402
from rllab.envs.normalized_env import normalize  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, FiniteDifferenceHvp  # noqa: E402
from rllab.policies.gaussian_gru_policy import GaussianGRUPolicy  # noqa: E402

# tools/exp/trpo_gru_cartpole_cpu.py (the CPU yardstick) and tests/test_gpu_gru.py run this very configuration
CONFIG = dict(batch_size=4000, max_path_length=100, n_itr=10, discount=0.99, step_size=0.01, hvp_base_eps=1e-5)


def make_algo(seed=1, n_itr=None, bptt_kernels=False):
    """``bptt_kernels``: the update on the recurrent HIP kernels (policies/fused_gru_ops.py) with the optimizer's default
    products, which are then the Fisher-vector kernel; the default is the configuration the yardstick ran."""
    ext.set_seed(seed)
    env = normalize(CartpoleEnv())
    policy = GaussianGRUPolicy(env_spec=env.spec, bptt_kernels=bptt_kernels)
    baseline = LinearFeatureBaseline(env_spec=env.spec)
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
                    help="loss, gradient and Fisher-vector products of the update on the recurrent HIP kernels")
    args = ap.parse_args()
    if args.csv:
        logger.add_tabular_output(args.csv)
    if args.quiet:
        logger.set_quiet(True)
    make_algo(args.seed, args.n_itr, args.bptt_kernels).train()


if __name__ == "__main__":
    main()
