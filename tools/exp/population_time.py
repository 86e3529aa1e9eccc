#!/usr/bin/env python
"""Time one population launch (rl_rollout_population) against the only way to do the same work without it: one
HipVecEnv.rollout launch per candidate on a 1-env executor.

  python tools/exp/population_time.py [--n-cand 4096] [--horizon 500] [--out profiles/population_time.json]

HIP events around every launch, 3 warm-up launches, the median of the repeated ones.  The per-candidate baseline is
measured over 64 candidates (each timed on its own) and EXTRAPOLATED to n_cand by multiplication."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-cand", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--baseline-candidates", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rllab_amd.envs.mujoco.swimmer_env import SwimmerEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    np.random.seed(0)
    env = normalize(SwimmerEnv())
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(args.hidden, args.hidden))
    lay = pol.kernel_layout()
    T, n = args.horizon, args.n_cand
    theta = pol.flat_params.detach().double()
    xs = theta[None, :] + 0.1 * torch.randn((n, theta.numel()), dtype=torch.float64, device=theta.device)
    rows = lay.pack_rows(xs.to(torch.float32))
    vec = env.vec_env_executor(n_envs=n, max_path_length=T, seed=1)
    res = dict(env="swimmer", hidden=[args.hidden] * 2, n_cand=n, n_evals=1, horizon=T, reps=args.reps,
               device=torch.cuda.get_device_name(0))
    for name, record in (("planes_off", False), ("planes_on", True)):
        med, lo, hi = timed(lambda: vec.rollout_population(rows, 1, T, 0.99, record=record), 3, args.reps)
        res["population_ms_" + name] = dict(median=med, min=lo, max=hi)
        print("population launch, %s: median %.3f ms (min %.3f, max %.3f)" % (name, med, lo, hi), flush=True)
    # the parent's way: set the candidate, roll it out alone
    one = env.vec_env_executor(n_envs=1, max_path_length=T, seed=1)
    plan = one.rollout_plan(pol, T)

    def one_candidate(c):
        pol.set_param_values(xs[c])
        one.rollout(pol, T)
    per = [timed(lambda: one_candidate(c), 1 if c else 3, 1)[0] for c in range(args.baseline_candidates)]
    res["per_candidate_rollout_ms"] = dict(median=float(np.median(per)), min=float(np.min(per)), max=float(np.max(per)),
                                           candidates=args.baseline_candidates,
                                           kernel=plan.name.decode() if plan is not None else None)
    res["per_candidate_extrapolated_ms"] = float(np.median(per)) * n
    print("one rollout launch per candidate (1-env executor): median %.3f ms over %d candidates -> %.1f ms extrapolated to %d"
          % (np.median(per), args.baseline_candidates, res["per_candidate_extrapolated_ms"], n), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
