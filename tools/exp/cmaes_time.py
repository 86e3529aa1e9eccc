#!/usr/bin/env python
"""Where the time of a CMA-ES iteration goes on the device.  HIP events, 3 warm-ups, the median of 11.

  1. rl_cmaes_cov_update against the torch composition of the same update (cov_update_torch) on the same device, at
     N = 1250 (the (32, 32) Cartpole policy, popsize 25: mu = mu_neg = 12) and N = 4546, with the bytes the pass has to move
     (4 N^2 8 B: C and _Yneg read and written once) over the kernel's time and over the HBM peak of 8.0 TB/s.
  2. One ask + rollout + tell of CMAES on Cartpole (32, 32) and the share of it that the eigendecomposition takes.

Writes profiles/cmaes_time.json.  Needs a HIP device: without one it fails.

  python tools/exp/cmaes_time.py [--out profiles/cmaes_time.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WARMUP, REPEATS, HBM_PEAK = 3, 11, 8.0e12


def timed(fn, prepare=None):
    """Median milliseconds of ``fn()`` between two events, after WARMUP calls; ``prepare`` runs untimed before each call."""
    ms = []
    for k in range(WARMUP + REPEATS):
        if prepare is not None:
            prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def cov_update_times(N):
    from rllab_amd.algos.cma_state import CMAParameters, cov_update_hip, cov_update_torch
    sp = CMAParameters(N)
    g = torch.Generator(device="cuda")
    g.manual_seed(N)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64, device="cuda")
    A = r(N, N)
    C0 = torch.matmul(A, A.t()) / N + torch.eye(N, dtype=torch.float64, device="cuda")
    Y0 = r(N, N)
    Y0 = Y0 + Y0.t()
    Ypos, Vneg, pc = r(sp.mu, N), r(sp.neg_mu, N), r(N)
    wpos = torch.as_tensor(sp.cmu * sp.weights, device="cuda")
    wneg = torch.as_tensor(sp.neg_weights, device="cuda")
    scal = torch.as_tensor([1 - sp.c1 - sp.cmu, sp.c1, 1 - sp.neg_cmuexp], dtype=torch.float64, device="cuda")
    C, Yn, dC = C0.clone(), Y0.clone(), torch.zeros(N, dtype=torch.float64, device="cuda")

    def reset():
        C.copy_(C0)
        Yn.copy_(Y0)
    out = {"N": N, "mu": sp.mu, "mu_neg": sp.neg_mu, "bytes": 4 * N * N * 8}
    for name, fn in (("hip", cov_update_hip), ("torch", cov_update_torch)):
        med, lo, hi = timed(lambda: fn(C, Yn, dC, Ypos, wpos, Vneg, wneg, pc, scal), prepare=reset)
        out[name + "_ms"] = {"median": med, "min": lo, "max": hi}
    out["hip_bytes_per_s"] = out["bytes"] / (out["hip_ms"]["median"] * 1e-3)
    out["hip_fraction_of_hbm_peak"] = out["hip_bytes_per_s"] / HBM_PEAK
    out["torch_over_hip"] = out["torch_ms"]["median"] / out["hip_ms"]["median"]
    return out


def iteration_times():
    """ask / rollout / tell of one CMAES iteration on Cartpole (32, 32), timed piecewise on a state a few iterations in."""
    from rllab_amd.algos import cma_state
    from rllab_amd.algos.cma_state import CMAState
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(1)
    env = normalize(CartpoleEnv())
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    layout = policy.kernel_layout()
    x0 = torch.as_tensor(policy.get_param_values(), dtype=torch.float64, device=policy.flat_params.device)
    es = CMAState(x0, 1.0, dict(seed=1))
    n, mpl = es.sp.popsize, 100
    vec_env = env.vec_env_executor(n_envs=n, max_path_length=mpl, seed=1)
    log_min_std = math.log(policy.min_std)
    box = {}

    def ask():
        box["xs"] = es.ask()

    def rollout():
        rows = layout.pack_rows(box["xs"].to(torch.float32))
        _, fp = vec_env.rollout_population(rows, 1, mpl, 0.99, record=False, layer_activations=layout.layer_activations,
                                           log_min_std=log_min_std)
        box["fs"] = -fp[0].to(torch.float64)

    def tell():
        es.tell(box["xs"], box["fs"])

    def eigh():
        cma_state.eigh(es.C)
    ms = {"ask": [], "rollout": [], "tell": [], "eigh": []}
    for k in range(WARMUP + REPEATS):
        for name, fn in (("ask", ask), ("rollout", rollout), ("tell", tell), ("eigh", eigh)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                ms[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    vec_env.terminate()
    # The lazy criterion updates B and D every 1 / (c1 + cmu) / N / 10 iterations (about 5 at N = 1250), so the median ask
    # holds no eigendecomposition; "eigh" is that call alone, and an average iteration pays it at the rate the run showed.
    rate = es.count_eigen / float(es.countiter)
    without = med["ask"] + med["rollout"] + med["tell"]
    total = without + rate * med["eigh"]
    return {"N": es.N, "popsize": n, "max_path_length": mpl, "ms": med, "iteration_ms_without_eigh": without,
            "eigendecompositions": es.count_eigen, "iterations": es.countiter, "eigh_per_iteration": rate,
            "average_iteration_ms": total, "eigh_share_of_average_iteration": rate * med["eigh"] / total,
            "eigh_path": cma_state.eigh_path("cuda")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmaes_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cmaes_time.py measures on a HIP device"
    result = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS,
              "cov_update": [cov_update_times(N) for N in (1250, 4546)], "iteration": iteration_times()}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
