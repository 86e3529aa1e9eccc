#!/usr/bin/env python
"""Train TRPO with a recurrent policy (GaussianGRUPolicy) on a partially observable Cartpole: the policy sees the two
positions only (OcclusionEnv, rows 0 and 2: no velocities) and its actions reach the cart two steps late
(DelayedActionEnv).  A feed-forward policy cannot recover either; the GRU carries both in its hidden state.

    env = normalize(DelayedActionEnv(OcclusionEnv(CartpoleEnv(), [0, 2]), action_delay=2))

Sampling stays one kernel launch per batch: the env kernels produce the full observation, the GRU's weight rows at the
occluded entries are zero (the batch keeps the rows the policy saw), and the action queue is an LDS ring inside the
recurrent rollout (rl_rollout_gaussian_gru_delayed).  With --bptt-kernels the update runs on the recurrent update kernels
(rl_gru_gaussian_eval / _grad / _fvp), otherwise through torch autograd with finite-difference products.

  python examples/trpo_gru_cartpole_po.py --bptt-kernels
  python examples/trpo_gru_cartpole_po.py --n-itr 20 --csv gru_cartpole_po.csv
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.trpo import TRPO  # noqa: E402
from rllab.baselines.linear_feature_baseline import LinearFeatureBaseline  # noqa: E402
from rllab.envs.box2d.cartpole_env import CartpoleEnv  # noqa: E402
from rllab.envs.noisy_env import DelayedActionEnv  # noqa: E402
from rllab.envs.normalized_env import normalize  # noqa: E402
from rllab.envs.occlusion_env import OcclusionEnv  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, FiniteDifferenceHvp  # noqa: E402
from rllab.policies.gaussian_gru_policy import GaussianGRUPolicy  # noqa: E402

# tests/test_gpu_partial_obs.py runs this very configuration (with bptt_kernels=True)
CONFIG = dict(batch_size=4000, max_path_length=100, n_itr=10, discount=0.99, step_size=0.01, hvp_base_eps=1e-5,
              sensor_idx=(0, 2), action_delay=2)


def make_env():
    return normalize(DelayedActionEnv(OcclusionEnv(CartpoleEnv(), list(CONFIG["sensor_idx"])),
                                      action_delay=CONFIG["action_delay"]))


def make_algo(seed=1, n_itr=None, bptt_kernels=True):
    ext.set_seed(seed)
    env = make_env()
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
