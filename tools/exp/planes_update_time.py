#!/usr/bin/env python
"""Time whole TRPO iterations of the two networks-on-planes policies, the sizes examples/run_trpo.py and
examples/trpo_gridworld.py run by default:

  adaptive_std : GaussianMLPPolicy(adaptive_std=True) on normalize(CartpoleEnv()), 1024 envs x 100 steps (FusedAdaptiveStdOps)
  categorical  : CategoricalMLPPolicy on GridWorldEnv("4x4"), 80 envs x 50 steps (FusedCategoricalOps)

  python tools/exp/planes_update_time.py [--root DIR] [--warmup 3] [--reps 15] [--out FILE.json]

``--root`` names the tree whose ``rllab_amd`` is timed (default: the one this file is in), so that two builds can be run one
after the other on the same box by the same script.  An iteration is obtain_samples + process_samples + optimize_policy;
wall clock around work that ends in a device synchronise (the update is bound by what the host does between its launches,
which device events alone would not show), warm-up iterations first, per-iteration times and the ``optimize_policy`` share
out.  Needs a HIP device."""
import argparse
import json
import os
import sys
import time

import numpy as np


def build(which):
    from rllab_amd.algos.trpo import TRPO
    from rllab_amd.baselines.linear_feature_baseline import LinearFeatureBaseline
    from rllab_amd.misc import ext
    ext.set_seed(1)
    if which == "adaptive_std":
        from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
        from rllab_amd.envs.normalized_env import normalize
        from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
        env, n, T = normalize(CartpoleEnv()), 1024, 100
        policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32), adaptive_std=True)
    else:
        from rllab_amd.envs.grid_world_env import GridWorldEnv
        from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
        env, n, T = GridWorldEnv("4x4"), 80, 50
        policy = CategoricalMLPPolicy(env_spec=env.spec)
    algo = TRPO(env=env, policy=policy, baseline=LinearFeatureBaseline(env_spec=env.spec), batch_size=n * T,
                max_path_length=T, n_itr=1, discount=0.99, step_size=0.01, sampler_args=dict(n_envs=n))
    algo.start_worker()
    algo.init_opt()
    return algo, dict(n_envs=n, horizon=T, ops=type(algo.optimizer._fused).__name__)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("planes_update_time.py measures on a HIP device; none is visible")
    import rllab_amd
    from rllab_amd.misc import logger
    assert os.path.dirname(os.path.dirname(os.path.abspath(rllab_amd.__file__))) == os.path.abspath(args.root)
    logger.set_quiet(True)
    res = dict(root=os.path.abspath(args.root), device=torch.cuda.get_device_name(0), warmup=args.warmup, reps=args.reps)
    for which in ("adaptive_std", "categorical"):
        algo, info = build(which)
        assert info["ops"] == dict(adaptive_std="FusedAdaptiveStdOps", categorical="FusedCategoricalOps")[which]
        iters, updates = [], []
        for itr in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samples = algo.sampler.process_samples(itr, algo.sampler.obtain_samples(itr))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            algo.optimize_policy(itr, samples)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            logger.dump_tabular()
            if itr >= args.warmup:
                iters.append((t2 - t0) * 1e3)
                updates.append((t2 - t1) * 1e3)
        res[which] = dict(info, iteration_ms=iters, update_ms=updates, iteration_median_ms=float(np.median(iters)),
                          update_median_ms=float(np.median(updates)))
        print("%-13s iteration median %8.3f ms, update median %8.3f ms over %d iterations"
              % (which, np.median(iters), np.median(updates), len(iters)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
