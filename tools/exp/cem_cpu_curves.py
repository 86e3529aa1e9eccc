#!/usr/bin/env python
"""CEM on the CPU, the yardstick of tests/test_gpu_cem.py::test_cem_learns_cartpole: the loop of rllab/algos/cem.py:107-181
with the reference's defaults (n_samples=100, max_path_length=500, discount 0.99, init_std = extra_std = 1, best_frac 0.05)
on normalize(CartpoleEnv()) -- the host build of the env (oracle.host_env, float64), a float64 numpy policy, and the
algorithm's own cem_scores / cem_refit / cem_sample_std.  No GPU.  Writes one row per (seed, iteration).

  python tools/exp/cem_cpu_curves.py --n-itr 8 --csv profiles/curves/cem_cartpole_cpu.csv
"""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import host_env as H  # noqa: E402
from rllab_amd.algos.cem import cem_refit, cem_sample_std, cem_scores  # noqa: E402

KIND, DO, DA, HID = 0, 4, 1, 32


def mean_action(x, o):
    """(32, 32) tanh MLP of the flat vector x (W0, b0, W1, b1, Wout, bout, log_std; W stored [in, out]) at observation o."""
    k = 0
    h = o
    for i, j in ((DO, HID), (HID, HID)):
        W = x[k:k + i * j].reshape(i, j); k += i * j
        h = np.tanh(h @ W + x[k:k + j]); k += j
    W = x[k:k + HID * DA].reshape(HID, DA); k += HID * DA
    return h @ W + x[k:k + DA], x[k + DA:k + 2 * DA]


def rollout(x, rng, max_path_length, discount, min_std=1e-6):
    env = H.HostEnv(KIND, np.float64, normalize=True)
    o = env.reset(rng.rand(4))
    disc, und, g, t = 0.0, 0.0, 1.0, 0
    while t < max_path_length:
        mean, log_std = mean_action(x, o)
        a = mean + rng.randn(DA) * np.exp(np.maximum(log_std, np.log(min_std)))
        o, r, d = env.step(a)
        disc += g * r; und += r; g *= discount; t += 1
        if d:
            break
    return disc, und, t


def run(seed, n_itr, n_samples=100, max_path_length=500, discount=0.99, init_std=1.0, best_frac=0.05, extra_std=1.0,
        extra_decay_time=100):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    from rllab_amd.spaces import Box
    ext.set_seed(seed)
    rng = np.random.RandomState(seed)
    spec = EnvSpec(Box(-1e6 * np.ones(DO), 1e6 * np.ones(DO)), Box(-np.ones(DA), np.ones(DA)))
    cur_mean = torch.as_tensor(GaussianMLPPolicy(spec, hidden_sizes=(HID, HID)).get_param_values())
    cur_std = torch.full_like(cur_mean, init_std)
    n_best = max(1, int(n_samples * best_frac))
    rows = []
    for itr in range(n_itr):
        sample_std = cem_sample_std(cur_std, extra_std, itr, extra_decay_time)
        xs = torch.as_tensor(rng.randn(n_samples, cur_mean.numel())) * sample_std + cur_mean
        fp = np.array([rollout(x, rng, max_path_length, discount) for x in xs.numpy()]).T          # [3, n_samples]
        fs, und = cem_scores(torch.as_tensor(fp), n_samples, 1)
        cur_mean, cur_std, _, _ = cem_refit(xs, fs, n_best)
        rows.append(dict(Seed=seed, Iteration=itr, CurStdMean=float(cur_std.mean()), AverageReturn=float(und.mean()),
                         MaxReturn=float(und.max()), MinReturn=float(und.min()), AverageDiscountedReturn=float(fs.mean()),
                         AvgTrajLen=float(fp[2].mean())))
        print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-itr", type=int, default=8)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3, 4, 5])
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    rows = [r for s in args.seeds for r in run(s, args.n_itr)]
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(rows)


if __name__ == "__main__":
    main()
