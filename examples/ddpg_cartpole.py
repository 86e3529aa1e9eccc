#!/usr/bin/env python
"""Train DDPG on Cartpole (the body of rllab's examples/ddpg_cartpole.py).

``--n-envs`` copies of the env collect in lock step into a replay pool on the device; every step is followed by
``n_envs`` updates -- batch draws, target values, the Q step, the policy step and the soft target updates -- in one
kernel launch.

  python examples/ddpg_cartpole.py
  python examples/ddpg_cartpole.py --n-envs 8 --n-epochs 50 --csv ddpg.csv
  python examples/ddpg_cartpole.py --n-envs 64 --rollout-steps 10      (collection and evaluation in the fused rollout)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rllab.algos.ddpg import DDPG  # noqa: E402
from rllab.envs.box2d.cartpole_env import CartpoleEnv  # noqa: E402
from rllab.envs.normalized_env import normalize  # noqa: E402
from rllab.exploration_strategies.ou_strategy import OUStrategy  # noqa: E402
from rllab.misc import ext, logger  # noqa: E402
from rllab.policies.deterministic_mlp_policy import DeterministicMLPPolicy  # noqa: E402
from rllab.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1)
    ap.add_argument("--rollout-steps", type=int, default=None,
                    help="collect in launches of the fused rollout of this many lock-steps (default: one transition "
                         "at a time)")
    ap.add_argument("--n-epochs", type=int, default=1000)
    ap.add_argument("--epoch-length", type=int, default=1000)
    ap.add_argument("--min-pool-size", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--csv", default=None, help="write the tabular log (one row per epoch) to this file")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    if args.csv:
        logger.add_tabular_output(args.csv)
    if args.quiet:
        logger.set_quiet(True)
    ext.set_seed(args.seed)
    env = normalize(CartpoleEnv())
    policy = DeterministicMLPPolicy(
        env_spec=env.spec,
        # The neural network policy should have two hidden layers, each with 32 hidden units.
        hidden_sizes=(32, 32)
    )
    es = OUStrategy(env_spec=env.spec)
    qf = ContinuousMLPQFunction(env_spec=env.spec)
    algo = DDPG(
        env=env,
        policy=policy,
        es=es,
        qf=qf,
        batch_size=32,
        max_path_length=100,
        epoch_length=args.epoch_length,
        min_pool_size=args.min_pool_size,
        n_epochs=args.n_epochs,
        discount=0.99,
        scale_reward=0.01,
        qf_learning_rate=1e-3,
        policy_learning_rate=1e-4,
        n_envs=args.n_envs,
        rollout_steps=args.rollout_steps,
    )
    algo.train()


if __name__ == "__main__":
    main()
