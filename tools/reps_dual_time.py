#!/usr/bin/env python
"""Timings of the REPS dual on an MI355X (HIP events on the launch stream; needs the GPU).

* rl_reps_dual (both launches) and rl_reps_weights on real batches at 500 x 4096 Swimmer and 500 x 1024 HalfCheetah:
  algorithmic bytes per sample 4 (Do + 1) + 4 + 1 + 1 (+ 4 written by the weights), achieved TB/s and its share of the
  8 TB/s HBM peak;
* the torch definition's dual (rllab_amd/algos/reps.py, float64, feature differences built once outside the timed
  region) on the same device and batch -- the only baseline there is;
* one full REPS iteration next to one TRPO iteration of the same configuration (host clock around work that ends in a
  device synchronise).

  python tools/reps_dual_time.py --out profiles/reps_dual_time.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def event_ms(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def make_algo(cls, env_name, n_envs, hidden, **kw):
    from rllab_amd.baselines.linear_feature_baseline import LinearFeatureBaseline
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(1)
    if env_name == "swimmer":
        from rllab_amd.envs.mujoco.swimmer_env import SwimmerEnv
        env = normalize(SwimmerEnv())
    else:
        from rllab_amd.envs.mujoco.half_cheetah_env import HalfCheetahEnv
        env = normalize(HalfCheetahEnv())
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=hidden)
    return cls(env=env, policy=policy, baseline=LinearFeatureBaseline(env_spec=env.spec), batch_size=n_envs * 500,
               max_path_length=500, discount=0.99, sampler_args=dict(n_envs=n_envs), **kw)


def iteration_ms(algo, iters, warm):
    """Mean wall time of obtain_samples -> process_samples -> optimize_policy, device idle at both ends."""
    from rllab_amd.misc import logger
    times = []
    for itr in range(warm + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = algo.sampler.obtain_samples(itr)
        sd = algo.sampler.process_samples(itr, paths)
        algo.optimize_policy(itr, sd)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        logger.dump_tabular()
    return float(np.mean(times[warm:])), float(np.std(times[warm:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--algo-iters", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run cannot give a time"
    from rllab_amd.algos import reps as R
    from rllab_amd.algos.trpo import TRPO
    from rllab_amd.misc import logger
    logger.set_quiet(True)
    results = []
    for env_name, n_envs, hidden in (("swimmer", 4096, (32, 32)), ("half_cheetah", 1024, (64, 64))):
        algo = make_algo(R.REPS, env_name, n_envs, hidden, n_itr=1)
        algo.start_worker()
        algo.init_opt()
        sd = algo.sampler.process_samples(0, algo.sampler.obtain_samples(0))
        traj = sd["_traj"]
        Do, B = traj.obs_dim, traj.B
        k = R.FusedRepsDual(traj)
        v = np.random.RandomState(0).rand(2 * Do + 4)
        eta = 15.0
        ms_dual = event_ms(lambda: k.launch(eta, v), args.iters, 5)
        w = [None]

        def weights_only():
            # (weights() launches the dual first; time the pair and subtract)
            w[0] = k.weights(eta, v)
        ms_pair = event_ms(weights_only, args.iters, 5)
        fd = R.reps_feat_diff(traj.obs, traj.tin, traj.dones, traj.valid)
        ms_def = event_ms(lambda: R.reps_dual_sums(eta, v, traj.rewards, fd, traj.valid), max(3, args.iters // 10), 2)
        del fd
        bytes_dual = B * (4 * (Do + 1) + 4 + 1 + 1)
        row = dict(env=env_name, T=traj.T, N=traj.N, obs_dim=Do, samples=B,
                   dual_ms=round(ms_dual, 4), dual_bytes=bytes_dual, dual_TBps=round(bytes_dual / ms_dual / 1e9, 3),
                   dual_frac_hbm_peak=round(bytes_dual / (ms_dual * 1e-3) / HBM_PEAK, 3),
                   weights_ms=round(ms_pair - ms_dual, 4), weights_bytes=bytes_dual + 4 * B,
                   definition_dual_ms=round(ms_def, 3), definition_over_kernel=round(ms_def / ms_dual, 1))
        reps_ms, reps_sd = iteration_ms(algo, args.algo_iters, 2)
        algo.shutdown_worker()
        trpo = make_algo(TRPO, env_name, n_envs, hidden, n_itr=1, step_size=0.01)
        trpo.start_worker()
        trpo.init_opt()
        trpo_ms, trpo_sd = iteration_ms(trpo, args.algo_iters, 2)
        trpo.shutdown_worker()
        row.update(reps_iteration_ms=round(reps_ms, 2), reps_iteration_std=round(reps_sd, 2),
                   trpo_iteration_ms=round(trpo_ms, 2), trpo_iteration_std=round(trpo_sd, 2))
        print(json.dumps(row))
        results.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_peak_TBps=HBM_PEAK / 1e12, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
