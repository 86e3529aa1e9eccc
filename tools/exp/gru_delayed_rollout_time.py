#!/usr/bin/env python
"""Time the fused recurrent rollout under DelayedActionEnv (rl_rollout_gaussian_gru_delayed, action_delay 3) next to the
plain one (rl_rollout_gaussian_gru): GaussianGRUPolicy with 32 units on normalize(CartpoleEnv()), 4096 envs x 100 steps
each, the two alternating in one process.

  python tools/exp/gru_delayed_rollout_time.py [--out profiles/gru_delayed_rollout_time.json]

HIP events around every launch (plane allocation included, as in a sampler's launch), warm-up launches of both first, then
``--reps`` rounds of (one delayed launch, one plain launch); the median, minimum and maximum of each and the ratio of the
medians.  A record, not a gate.  Needs a HIP device."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_delayed_rollout_time.py measures on a HIP device; none is visible")
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.noisy_env import DelayedActionEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    np.random.seed(0)
    plain_env = normalize(CartpoleEnv())
    delayed_env = normalize(DelayedActionEnv(CartpoleEnv(), action_delay=args.delay))
    gru = GaussianGRUPolicy(plain_env.spec, hidden_sizes=(32,))
    n, T = args.n_envs, args.horizon
    v_plain = plain_env.vec_env_executor(n_envs=n, max_path_length=T, seed=1)
    v_delay = delayed_env.vec_env_executor(n_envs=n, max_path_length=T, seed=1)
    assert v_plain.takes_rollout_of(gru) and v_delay.takes_rollout_of(gru) and v_delay.action_delay == args.delay
    launches = (("delayed", lambda: v_delay.rollout(gru, T)), ("plain", lambda: v_plain.rollout(gru, T)))
    for _ in range(args.warmup):
        for _, fn in launches:
            fn()
    torch.cuda.synchronize()
    ms = dict(delayed=[], plain=[])
    for _ in range(args.reps):
        for name, fn in launches:
            ms[name].append(one(fn))
    res = dict(env="cartpole", hidden=32, n_envs=n, horizon=T, action_delay=args.delay, warmup=args.warmup, reps=args.reps,
               device=torch.cuda.get_device_name(0))
    for name in ("delayed", "plain"):
        x = np.array(ms[name])
        res[name + "_ms"] = dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))
        res[name + "_env_steps_per_s"] = float(n * T / (np.median(x) * 1e-3))
        print("%s rollout, %d envs x %d steps: median %.3f ms (min %.3f, max %.3f) over %d launches" % (
            name, n, T, np.median(x), x.min(), x.max(), x.size), flush=True)
    res["delayed_over_plain"] = float(np.median(ms["delayed"]) / np.median(ms["plain"]))
    print("delayed / plain = %.4f" % res["delayed_over_plain"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
