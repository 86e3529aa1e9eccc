#!/usr/bin/env python
"""Timings of the fused DDPG update on an MI355X (HIP events on the launch stream; needs the GPU).

Per shape -- (obs 4, act 1, hidden (32, 32)) and (obs 21, act 6, hidden (64, 64)), batch 32, Adam on both nets, a pool
of 65 536 rows, batches drawn in the kernel -- the median of 7 measurements of

* rl_ddpg_update per update at K = 1, 64 and 1024 updates per launch (a measurement = several launches back to back
  between two events, divided by launches x K);
* the same update as float32 torch eager on the same device, per update: target values, the Q step and the policy step
  by autograd, Adam and the soft target updates as tensor expressions, batch rows from torch.randint -- the only
  baseline there is (the reference's Theano functions do not run here).

  python tools/ddpg_update_time.py --out profiles/ddpg_update_time.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(4, 1, (32, 32), 32), (21, 6, (64, 64), 32)]
LAUNCHES = {1: 200, 64: 20, 1024: 3}
POOL_ROWS = 65536
HYPER = dict(discount=0.99, tau=1e-3, qf_learning_rate=1e-3, policy_learning_rate=1e-4)


def median_of(fn, n=7):
    return float(np.median([fn() for _ in range(n)]))


def event_us(fn, iters):
    """Microseconds per call of ``fn`` over ``iters`` calls between two events."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


class EagerUpdate(object):
    """One DDPG update as float32 torch expressions on the device (the arithmetic of rl_ddpg_update, Adam on both nets)."""

    def __init__(self, policy, qf, pool, batch):
        self.policy, self.qf, self.pool, self.batch = policy, qf, pool, batch
        c = lambda t: t.detach().clone()
        self.pi, self.q = c(policy.flat_params), c(qf.flat_params)
        self.tpi, self.tq = c(self.pi), c(self.q)
        self.mom = [torch.zeros_like(x) for x in (self.pi, self.pi, self.q, self.q)]
        self.t = 0
        wm = lambda obj: torch.cat([torch.full((p.size,), float(p.tags["regularizable"]), device=self.pi.device)
                                    for p in obj.get_params()])
        self.wm_pi, self.wm_q = wm(policy), wm(qf)

    def _adam(self, theta, g, m, v, lr):
        a_t = lr * np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t)
        m.mul_(0.9).add_(g, alpha=0.1)
        v.mul_(0.999).addcmul_(g, g, value=0.001)
        return theta - a_t * m / (torch.sqrt(v) + 1e-8)

    def __call__(self):
        p = self.pool
        rows = torch.randint(0, p.size, (self.batch,), device=self.pi.device)
        s, a, r, term, s2 = p.obs[rows], p.act[rows], p.rew[rows], p.term[rows], p.next_obs[rows]
        self.t += 1
        with torch.no_grad():
            y = r + (1.0 - term) * HYPER["discount"] * self.qf.get_qval_sym(s2, self.policy.get_action_sym(s2, self.tpi),
                                                                           self.tq)
        qv = self.q.requires_grad_(True)
        loss = ((y - self.qf.get_qval_sym(s, a, qv)) ** 2).mean()
        g = torch.autograd.grad(loss, qv)[0]
        self.q = self._adam(self.q.detach(), g, self.mom[2], self.mom[3], HYPER["qf_learning_rate"])
        pv = self.pi.requires_grad_(True)
        surr = -self.qf.get_qval_sym(s, self.policy.get_action_sym(s, pv), self.q).mean()
        g = torch.autograd.grad(surr, pv)[0]
        self.pi = self._adam(self.pi.detach(), g, self.mom[0], self.mom[1], HYPER["policy_learning_rate"])
        tau = HYPER["tau"]
        self.tpi = self.tpi * (1.0 - tau) + self.pi * tau
        self.tq = self.tq * (1.0 - tau) + self.q * tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--eager-updates", type=int, default=50)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    assert torch.cuda.is_available(), "needs a HIP device: a CPU run cannot give a time"
    from rllab_amd.algos.ddpg_update import FusedDDPGUpdate
    from rllab_amd.algos.replay_pool import DeviceReplayPool
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab_amd.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    from rllab_amd.spaces import Box
    results = []
    for D, A, hs, B in SHAPES:
        np.random.seed(1)
        torch.manual_seed(1)
        spec = EnvSpec(Box(-1e6 * np.ones(D), 1e6 * np.ones(D)), Box(-np.ones(A), np.ones(A)))
        policy, qf = DeterministicMLPPolicy(spec, hidden_sizes=hs), ContinuousMLPQFunction(spec, hidden_sizes=hs)
        pool = DeviceReplayPool(POOL_ROWS, D, A)
        n = POOL_ROWS
        dev = pool.device
        pool.add(torch.randn(n, D, device=dev), torch.rand(n, A, device=dev) * 2 - 1, torch.randn(n, device=dev),
                 torch.rand(n, device=dev) < 0.02, torch.randn(n, D, device=dev))
        upd = FusedDDPGUpdate(policy, qf, B)
        row = dict(obs_dim=D, act_dim=A, hidden=list(hs), batch=B, pool_rows=n)
        base = [0]
        for K, launches in LAUNCHES.items():
            def launch():
                upd.update(pool, K, seed=7, update_base=base[0], **HYPER)
                base[0] += K
            launch()                                         # warm-up of the shape
            per_launch = median_of(lambda: event_us(launch, launches))
            row["fused_us_per_update_K%d" % K] = round(per_launch / K, 3)
            row["fused_us_per_launch_K%d" % K] = round(per_launch, 2)
        assert bool(torch.isfinite(upd.plane(0)).all())
        eager = EagerUpdate(policy, qf, pool, B)
        for _ in range(10):
            eager()
        row["torch_eager_us_per_update"] = round(median_of(lambda: event_us(eager, args.eager_updates)), 1)
        print(json.dumps(row))
        results.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), median_of=7, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
