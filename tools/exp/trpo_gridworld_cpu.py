#!/usr/bin/env python
"""TRPO on GridWorld on the CPU, the yardstick of tests/test_gpu_categorical.py::test_trpo_learns_gridworld: the Python
GridWorldEnv sampled one path after another by the reference's rollout loop (rllab/sampler/utils.py:5-40,
parallel_sampler.py:98-126: whole paths until batch_size samples are in), the reference's process_samples
(rllab/sampler/base.py:48-104: LinearFeatureBaseline, GAE with lambda = 1, centred advantages) in numpy, and the update
by this tree's ConjugateGradientOptimizer on float64 torch closures of the Categorical formulas (autograd gradient,
PerlmutterHvp products) -- none of the HIP kernels.  No GPU.  Writes one row per iteration.

  python tools/exp/trpo_gridworld_cpu.py --csv profiles/curves/trpo_gridworld_cpu.csv
"""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def discount_cumsum(x, discount):
    out, run = np.zeros(len(x)), 0.0
    for t in range(len(x) - 1, -1, -1):
        run = x[t] + discount * run
        out[t] = run
    return out


def sample_paths(env, policy, batch_size, max_path_length):
    """Whole paths until ``batch_size`` samples are in (the policy's table is read once per batch: observations are
    one-hot, so ``get_action`` is a row lookup followed by ``Discrete.weighted_sample``)."""
    S = env.observation_space.n
    table = policy.dist_info(np.eye(S))["prob"]
    paths, n = [], 0
    while n < batch_size:
        obs, acts, rews, probs = [], [], [], []
        o = env.reset()
        for _ in range(max_path_length):
            prob = table[o]
            a = env.action_space.weighted_sample(prob)
            o2, r, d, _ = env.step(a)
            obs.append(env.observation_space.flatten(o))
            acts.append(env.action_space.flatten(a))
            rews.append(r)
            probs.append(prob)
            o = o2
            if d:
                break
        paths.append(dict(observations=np.array(obs), actions=np.array(acts), rewards=np.array(rews, dtype=np.float64),
                          agent_infos=dict(prob=np.array(probs))))
        n += len(rews)
    return paths


def run(seed, n_itr, batch_size, max_path_length, desc="4x4", discount=0.99, step_size=0.01, hidden=(32, 32)):
    from rllab_amd.baselines.linear_feature_baseline import LinearFeatureBaseline
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import ext, logger
    from rllab_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer
    from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
    logger.set_quiet(True)
    ext.set_seed(seed)
    env = GridWorldEnv(desc)
    policy = CategoricalMLPPolicy(env_spec=env.spec, hidden_sizes=hidden)
    policy.flat_params = policy.flat_params.cpu().double()          # the float64 torch path
    dist = policy.distribution
    baseline = LinearFeatureBaseline(env_spec=env.spec)

    def surr_loss(flat, obs, act, adv, old_prob):
        lr = dist.likelihood_ratio_sym(act, dict(prob=old_prob), policy.dist_info_planes(obs, flat), axis=0)
        return -(lr * adv).mean()

    def mean_kl(flat, obs, act, adv, old_prob):
        return dist.kl_sym(dict(prob=old_prob), policy.dist_info_planes(obs, flat), axis=0).mean()

    opt = ConjugateGradientOptimizer()
    opt.update_opt(loss=surr_loss, target=policy, leq_constraint=(mean_kl, step_size), constraint_name="mean_kl")
    rows = []
    for itr in range(n_itr):
        paths = sample_paths(env, policy, batch_size, max_path_length)
        for p in paths:
            b = np.append(baseline.predict(p), 0)
            deltas = p["rewards"] + discount * b[1:] - b[:-1]
            p["advantages"] = discount_cumsum(deltas, discount)          # gae_lambda = 1
            p["returns"] = discount_cumsum(p["rewards"], discount)
        adv = np.concatenate([p["advantages"] for p in paths])
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        baseline.fit(paths)
        t = lambda key: torch.as_tensor(np.concatenate([p[key] for p in paths]).T.copy(), dtype=torch.float64)
        inputs = (t("observations"), t("actions"), torch.as_tensor(adv),
                  torch.as_tensor(np.concatenate([p["agent_infos"]["prob"] for p in paths]).T.copy()))
        opt.optimize(inputs)
        loss_before, kl_before = opt.last_before
        rows.append(dict(Seed=seed, Iteration=itr, AverageReturn=float(np.mean([p["rewards"].sum() for p in paths])),
                         NumTrajs=len(paths), LossBefore=loss_before, LossAfter=opt.loss(inputs),
                         MeanKLBefore=kl_before, MeanKL=opt.constraint_val(inputs)))
        print("seed %d itr %2d  AverageReturn %.4f  paths %d  MeanKL %.5f" % (
            seed, itr, rows[-1]["AverageReturn"], len(paths), rows[-1]["MeanKL"]), file=sys.stderr)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--n-itr", type=int, default=15)
    ap.add_argument("--batch-size", type=int, default=4000)
    ap.add_argument("--max-path-length", type=int, default=50)
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    rows = run(args.seed, args.n_itr, args.batch_size, args.max_path_length)
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(rows)


if __name__ == "__main__":
    main()
