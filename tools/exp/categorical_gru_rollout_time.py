#!/usr/bin/env python
"""Time the fused recurrent GridWorld rollout (rl_rollout_gridworld_gru, CategoricalGRUPolicy hidden 32) next to the
table rollout of a (32, 32) CategoricalMLPPolicy (rl_rollout_gridworld) on GridWorldEnv('4x4'): 4096 envs x 100 steps
each, the two alternating in one process.

  python tools/exp/categorical_gru_rollout_time.py [--n-envs 4096] [--horizon 100] [--out profiles/categorical_gru_rollout_time.json]

HIP events around every launch (plane allocation included, as in a sampler's launch; the MLP's probability table is built
once, before the clock, as a sampler builds it once per parameter version), warm-up launches of both first, then ``--reps``
rounds of (one GRU launch, one table launch); the median, minimum and maximum of each.  Needs a HIP device."""
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
    ap.add_argument("--desc", default="4x4")
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("categorical_gru_rollout_time.py measures on a HIP device; none is visible")
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
    np.random.seed(0)
    env = GridWorldEnv(args.desc)
    gru = CategoricalGRUPolicy(env.spec, hidden_dim=args.hidden)
    mlp = CategoricalMLPPolicy(env.spec, hidden_sizes=(32, 32))
    n, T = args.n_envs, args.horizon
    v_gru = env.vec_env_executor(n_envs=n, max_path_length=T, seed=1)
    v_mlp = env.vec_env_executor(n_envs=n, max_path_length=T, seed=1)
    assert v_gru.takes_rollout_of(gru) and v_mlp.takes_rollout_of(mlp)
    mlp.prob_table()
    launches = (("gru", lambda: v_gru.rollout(gru, T)), ("table", lambda: v_mlp.rollout(mlp, T)))
    for _ in range(args.warmup):
        for _, fn in launches:
            fn()
    torch.cuda.synchronize()
    ms = dict(gru=[], table=[])
    for _ in range(args.reps):
        for name, fn in launches:
            ms[name].append(one(fn))
    res = dict(env="gridworld " + args.desc, n_envs=n, horizon=T, warmup=args.warmup, reps=args.reps,
               device=torch.cuda.get_device_name(0), gru_lds_bytes=gru.kernel_lds_bytes())
    for name, label in (("gru", "gru_hidden%d" % args.hidden), ("table", "table_mlp_32_32")):
        x = np.array(ms[name])
        res[label + "_ms"] = dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))
        res[label + "_env_steps_per_s"] = float(n * T / (np.median(x) * 1e-3))
        print("%s rollout, %d envs x %d steps: median %.3f ms (min %.3f, max %.3f) over %d launches" % (
            label, n, T, np.median(x), x.min(), x.max(), x.size), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
