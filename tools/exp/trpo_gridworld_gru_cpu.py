#!/usr/bin/env python
"""TRPO on GridWorld with a CategoricalGRUPolicy on the CPU, the yardstick of
tests/test_gpu_categorical_gru.py::test_trpo_learns_gridworld_with_a_gru_policy: the configuration of
examples/trpo_gridworld_gru.py on the Python GridWorldEnv sampled one path after another by the reference's rollout loop
(rllab/sampler/utils.py:5-40 with agent.reset() per path, parallel_sampler.py:98-126: whole paths until batch_size samples
are in) with the policy's host ``get_action``, the reference's process_samples (rllab/sampler/base.py:48-161:
LinearFeatureBaseline, GAE with lambda = 1, centred advantages, paths padded to [paths, max_path_length] with ``valids``) in
numpy, and the update by this tree's ConjugateGradientOptimizer (FiniteDifferenceHvp, base_eps 1e-5) on float64 torch
closures of ``CategoricalGRUPolicy.dist_info_planes`` -- none of the HIP kernels.  No GPU.  Writes one row per iteration.
Returns are success rates in [0, 1].

  python tools/exp/trpo_gridworld_gru_cpu.py --csv profiles/curves/trpo_gridworld_gru_cpu.csv
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
    """Whole paths until ``batch_size`` samples are in; ``policy.reset()`` before every path, ``get_action`` per step (one
    np.random uniform each)."""
    paths, n = [], 0
    while n < batch_size:
        o = env.reset()
        policy.reset()
        obs, acts, rews, probs = [], [], [], []
        for _ in range(max_path_length):
            a, info = policy.get_action(o)
            obs.append(env.observation_space.flatten(o))
            acts.append(env.action_space.flatten(a))
            probs.append(info["prob"])
            o, r, d, _ = env.step(a)
            rews.append(float(r))
            if d:
                break
        paths.append(dict(observations=np.array(obs), actions=np.array(acts), rewards=np.array(rews),
                          agent_infos=dict(prob=np.array(probs))))
        n += len(rews)
    return paths


def padded(paths, key, T, sub=None):
    """[D, T, n_paths] float64 planes of a per-step array, zero behind a path's end."""
    rows = [(p[sub][key] if sub else p[key]) for p in paths]
    d = 1 if rows[0].ndim == 1 else rows[0].shape[1]
    out = np.zeros((d, T, len(paths)))
    for i, r in enumerate(rows):
        out[:, :len(r), i] = r.reshape(len(r), d).T
    return torch.as_tensor(out)


def run(seed, n_itr=None, **override):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from trpo_gridworld_gru import CONFIG
    from rllab_amd.baselines.linear_feature_baseline import LinearFeatureBaseline
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import ext, logger
    from rllab_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, FiniteDifferenceHvp
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    cfg = dict(CONFIG, **{k: v for k, v in override.items() if v is not None})
    logger.set_quiet(True)
    ext.set_seed(seed)
    n_itr = cfg["n_itr"] if n_itr is None else n_itr
    discount, T = cfg["discount"], cfg["max_path_length"]
    env = GridWorldEnv(cfg["desc"])
    policy = CategoricalGRUPolicy(env_spec=env.spec)
    policy.flat_params = policy.flat_params.cpu().double()          # the float64 torch path
    dist = policy.distribution
    baseline = LinearFeatureBaseline(env_spec=env.spec)

    def surr_loss(flat, obs, act, adv, old_prob, start, valid):
        new = policy.dist_info_planes(obs, act, start, flat)
        lr = dist.likelihood_ratio_sym(act, dict(prob=old_prob), new, axis=0)
        return -(lr * adv * valid).sum() / valid.sum()

    def mean_kl(flat, obs, act, adv, old_prob, start, valid):
        kl = dist.kl_sym(dict(prob=old_prob), policy.dist_info_planes(obs, act, start, flat), axis=0)
        return (kl * valid).sum() / valid.sum()

    opt = ConjugateGradientOptimizer(hvp_approach=FiniteDifferenceHvp(base_eps=cfg["hvp_base_eps"]))
    opt.update_opt(loss=surr_loss, target=policy, leq_constraint=(mean_kl, cfg["step_size"]), constraint_name="mean_kl")
    rows = []
    for itr in range(n_itr):
        paths = sample_paths(env, policy, cfg["batch_size"], T)
        for p in paths:
            b = np.append(baseline.predict(p), 0)
            deltas = p["rewards"] + discount * b[1:] - b[:-1]
            p["advantages"] = discount_cumsum(deltas, discount)          # gae_lambda = 1
            p["returns"] = discount_cumsum(p["rewards"], discount)
        adv = np.concatenate([p["advantages"] for p in paths])
        mean_a, std_a = adv.mean(), adv.std()
        for p in paths:
            p["advantages"] = (p["advantages"] - mean_a) / (std_a + 1e-8)
        baseline.fit(paths)
        n = len(paths)
        valid = torch.zeros((T, n), dtype=torch.float64)
        for i, p in enumerate(paths):
            valid[:len(p["rewards"]), i] = 1.0
        start = torch.zeros((T, n), dtype=torch.bool)
        start[0] = True
        inputs = (padded(paths, "observations", T), padded(paths, "actions", T), padded(paths, "advantages", T)[0],
                  padded(paths, "prob", T, sub="agent_infos"), start, valid)
        opt.optimize(inputs)
        loss_before, kl_before = opt.last_before
        rows.append(dict(Seed=seed, Iteration=itr, AverageReturn=float(np.mean([p["rewards"].sum() for p in paths])),
                         NumTrajs=n, NumSamples=int(valid.sum()), LossBefore=loss_before, LossAfter=opt.loss(inputs),
                         MeanKLBefore=kl_before, MeanKL=opt.constraint_val(inputs)))
        print("seed %d itr %2d  AverageReturn %.4f  paths %d  MeanKL %.5f" % (
            seed, itr, rows[-1]["AverageReturn"], n, rows[-1]["MeanKL"]), file=sys.stderr)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--n-itr", type=int, default=None, help="default: the example's")
    ap.add_argument("--batch-size", type=int, default=None, help="default: the example's")
    ap.add_argument("--max-path-length", type=int, default=None, help="default: the example's")
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    rows = run(args.seed, args.n_itr, batch_size=args.batch_size, max_path_length=args.max_path_length)
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(rows)


if __name__ == "__main__":
    main()
