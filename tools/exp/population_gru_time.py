#!/usr/bin/env python
"""Time the recurrent population rollout (rl_rollout_population_gru, one GaussianGRUPolicy of 32 units per env) on
normalize(CartpoleEnv()), 4096 candidates x 100 steps, with and without the recording planes, and in the same process the
two launches it is made of: the recurrent rollout of ONE such policy on as many envs (rl_rollout_gaussian_gru: the same GRU
step, weights staged in LDS) and the population rollout of (32, 32) GaussianMLPPolicy candidates (rl_rollout_population: the
same per-lane weight reads, 1.4 K floats per step instead of 3.7 K).

  python tools/exp/population_gru_time.py [--n-envs 4096] [--horizon 100] [--out profiles/population_gru_rollout_time.json]

HIP events around every launch (plane allocation and the transposition of the population included, as in an algorithm's
launch), warm-up launches of all first, then ``--reps`` rounds of one launch each; the median, minimum and maximum of
each.  Needs a HIP device."""
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("population_gru_time.py measures on a HIP device; none is visible")
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    np.random.seed(0)
    env = normalize(CartpoleEnv())
    gru = GaussianGRUPolicy(env.spec, hidden_sizes=(32,))
    mlp = GaussianMLPPolicy(env.spec, hidden_sizes=(32, 32))
    n, T = args.n_envs, args.horizon
    gen = torch.Generator(device=gru.flat_params.device)
    gen.manual_seed(1)

    def population(policy):       # candidates 0.1 * randn around the initial policy: paths of mixed lengths
        theta = torch.as_tensor(policy.get_param_values(), dtype=torch.float32, device=gru.flat_params.device)
        return theta + 0.1 * torch.randn((n, theta.numel()), generator=gen, dtype=torch.float32, device=theta.device)

    rows_gru = gru.pack_rows(population(gru))
    layout = mlp.kernel_layout()
    rows_mlp = layout.pack_rows(population(mlp))
    v = {k: env.vec_env_executor(n_envs=n, max_path_length=T, seed=1) for k in ("pop_gru", "pop_gru_rec", "gru", "pop_mlp")}
    assert v["gru"].takes_rollout_of(gru)
    pop_gru = lambda rec, key: v[key].rollout_population_recurrent(rows_gru, 1, T, 0.99, gru.kernel_hidden,
                                                                    gru.state_include_action, record=rec)
    launches = (
        ("population_gru_hidden32_no_record", lambda: pop_gru(False, "pop_gru")),
        ("population_gru_hidden32_record", lambda: pop_gru(True, "pop_gru_rec")),
        ("gru_hidden32", lambda: v["gru"].rollout(gru, T)),
        ("population_mlp_32_32_no_record", lambda: v["pop_mlp"].rollout_population(
            rows_mlp, 1, T, 0.99, record=False, layer_activations=layout.layer_activations)),
    )
    for _ in range(args.warmup):
        for _, fn in launches:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in launches}
    for _ in range(args.reps):
        for name, fn in launches:
            ms[name].append(one(fn))
    res = dict(env="cartpole", n_envs=n, horizon=T, warmup=args.warmup, reps=args.reps,
               device=torch.cuda.get_device_name(0),
               weight_bytes_per_env_step=dict(population_gru_hidden32=4 * int(rows_gru.shape[1]),
                                              population_mlp_32_32=4 * int(rows_mlp.shape[1])))
    for name, _ in launches:
        x = np.array(ms[name])
        res[name + "_ms"] = dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))
        res[name + "_env_steps_per_s"] = float(n * T / (np.median(x) * 1e-3))
        print("%s, %d envs x %d steps: median %.3f ms (min %.3f, max %.3f) over %d launches" % (
            name, n, T, np.median(x), x.min(), x.max(), x.size), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
