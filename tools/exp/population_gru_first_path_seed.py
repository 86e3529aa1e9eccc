#!/usr/bin/env python
"""The CPU search behind FIRST_PATH_SEED of tests/test_gpu_population_gru.py::test_first_path_accumulators_gru: for every
seed, the test's own candidates (0.5 * randn around the seed's initial GaussianGRUPolicy, 32 units, Cartpole) and its own
injected draws replayed through the host env (oracle.host_env) with a numpy GRU, in float32 and in float64, counting how
many of the 70 first paths end before the forced done at the horizon.  No GPU.

  python tools/exp/population_gru_first_path_seed.py --seeds 100 --horizon 100
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N_CAND, N_EVALS = 35, 2
N = N_CAND * N_EVALS


def _noise(q, n, horizon, seed=1):
    rng = np.random.RandomState(seed)
    eps = rng.randn(q["act_dim"], horizon, n).astype(np.float32)
    draws = (rng.randn if q["reset_is_normal"] else rng.rand)(horizon + 1, q["reset_draws"], n).astype(np.float32)
    return eps, draws


def first_path_search(seeds, horizon):
    """{seed: (early in float32, early in float64)}: how many of the 70 first paths end before the forced done."""
    from oracle import host_env as H
    from rllab_amd import _lib
    kind, hid = 0, 32
    q = _lib.env_query(kind)
    do, da = q["obs_dim"], q["act_dim"]
    di = do + da
    eps, draws = _noise(q, N, horizon)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    out = {}
    for seed in seeds:
        _, xs, _ = candidates_host(kind, hid, seed)
        early = []
        for dt in (np.float32, np.float64):
            n_early = 0
            for i in range(N):
                x = xs[i % N_CAND].astype(dt)
                k = hid
                p = {}
                for g in "ruc":
                    p["x" + g] = x[k:k + di * hid].reshape(di, hid); k += di * hid
                    p["h" + g] = x[k:k + hid * hid].reshape(hid, hid); k += hid * hid
                    p["b" + g] = x[k:k + hid]; k += hid
                wo = x[k:k + hid * da].reshape(hid, da); k += hid * da
                bo = x[k:k + da]; k += da
                std = np.exp(x[k:k + da].astype(np.float64)).astype(np.float32).astype(dt)
                env = H.HostEnv(kind, dt, normalize=True)
                o = env.reset(draws[0, :, i])
                h, pa = x[:hid], np.zeros(da, dtype=dt)
                for t in range(horizon):
                    xin = np.concatenate([np.asarray(o, dtype=dt), pa])
                    r = sig(xin @ p["xr"] + h @ p["hr"] + p["br"])
                    u = sig(xin @ p["xu"] + h @ p["hu"] + p["bu"])
                    cc = np.tanh(xin @ p["xc"] + r * (h @ p["hc"]) + p["bc"])
                    h = (1 - u) * h + u * cc
                    a = (h @ wo + bo + eps[:, t, i].astype(dt) * std).astype(dt)
                    o, _, d = env.step(a)
                    pa = a
                    if d:
                        n_early += t < horizon - 1
                        break
            early.append(n_early)
        out[seed] = tuple(early)
        print(seed, out[seed], flush=True)
    return out


def candidates_host(kind, hid, seed, scale=0.5):
    """``_candidates`` without a device: the same draws."""
    from rllab_amd import _lib
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.spaces import Box
    q = _lib.env_query(kind)
    spec = EnvSpec(Box(-1e6 * np.ones(q["obs_dim"]), 1e6 * np.ones(q["obs_dim"])),
                   Box(-np.ones(q["act_dim"]), np.ones(q["act_dim"])))
    np.random.seed(seed)
    pol = GaussianGRUPolicy(spec, hidden_sizes=(hid,))
    theta = pol.get_param_values()
    xs = (theta[None, :] + scale * np.random.RandomState(seed + 1).randn(N_CAND, theta.size)).astype(np.float32)
    return pol, xs, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--horizon", type=int, default=100)
    args = ap.parse_args()
    found = first_path_search(range(args.seeds), args.horizon)
    print({s: e for s, e in found.items() if e[0] == e[1] and N / 4 <= e[0] < N})


if __name__ == "__main__":
    main()
