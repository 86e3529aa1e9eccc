"""Every output bit of the three env-per-lane rollouts (rl_rollout_gaussian_gru, rl_rollout_population,
rl_rollout_gridworld_gru), pinned: tests/golden/lane_rollouts.json holds, per case and per output array, the shape, the
dtype and a SHA-256 of the bytes, recorded by tools/make_golden_lane_rollouts.py with the library of the commit its header
names.  The parity tests of these kernels hold the means to 1e-5 of a float64 pass and replay the actions; a reordered sum
passes them.  This one does not: a digest that differs is a changed float operation, a changed Philox counter or a changed
contraction site, and never a reason to record again.

The shapes are the smallest at which these kernels can still go wrong: 70 envs (two workgroups, a partial last wavefront),
25 steps, paths short enough that every env is reset inside the launch."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_categorical_gru import _policy as _grid_policy, _uniforms
from tests.test_gpu_cem import N_CAND, N_EVALS, T as POP_T, _candidates, _launch
from tests.test_gpu_gru import MPL, N, T, _noise, _policy as _gru_policy

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lane_rollouts.json")
GRID_MPL = 6                    # below the 4x4 map's usual path length: paths end by the time limit as well as by hole / goal
PLANES = ("obs", "actions", "means", "rewards", "dones")
NOISY = dict(action_noise=0.1, obs_noise=0.05)


def _env_noise(q, n, horizon, seed=3):
    rng = np.random.RandomState(seed)
    return (rng.randn(horizon, q["act_dim"], n).astype(np.float32), rng.randn(horizon + 1, q["obs_dim"], n).astype(np.float32))


def _joined(chunks, names=PLANES):
    """The planes of consecutive launches, one after the other along the time axis."""
    return {k: torch.cat([getattr(c, k) for c in chunks], dim=getattr(chunks[0], k).dim() - 2) for k in names}


# -- rl_rollout_gaussian_gru ----------------------------------------------------------------------------------------------
def _gru(kind=0, hidden=32, include_action=True, cfg=None, inject=True, cut=None, seed=5):
    from rllab_amd.envs.hip_env import HipVecEnv
    pol = _gru_policy(kind, hidden, state_include_action=include_action)
    v = HipVecEnv(kind, N, MPL, normalize=True, seed=seed, cfg=cfg)
    kw = {}
    if inject:
        kw["eps"], kw["reset_draws"] = _noise(v.q, N, T)
    if cfg is not None:
        kw["action_noise_z"], kw["obs_noise_z"] = _env_noise(v.q, N, T)
    if cut is None:
        out = _joined([v.rollout(pol, T, **kw)])
    else:
        eps, draws = kw["eps"], kw["reset_draws"]             # [Da, T, n] and [T + 1, R, n]
        out = _joined([v.rollout(pol, cut, eps=eps[:, :cut], reset_draws=draws[:cut + 1]),
                       v.rollout(pol, T - cut, reset_at_start=False, eps=eps[:, cut:], reset_draws=draws[cut:])])
    out.update(state=v.state, ts=v.ts, last_obs=v._obs, hidden_state=v.hidden_state, prev_action=v.prev_action)
    return out


# -- rl_rollout_population ------------------------------------------------------------------------------------------------
def _population(kind=0, hidden=(32, 32), cfg=None, inject=True, record=True, seed=5):
    from rllab_amd.envs.hip_env import HipVecEnv
    pol, _, rows = _candidates(kind, hidden)
    n = N_CAND * N_EVALS
    v = HipVecEnv(kind, n, 11, normalize=True, seed=seed, cfg=cfg)
    kw = {}
    if inject:
        kw["eps"], kw["reset_draws"] = _noise(v.q, n, POP_T)
    if cfg is not None:
        kw["action_noise_z"], kw["obs_noise_z"] = _env_noise(v.q, n, POP_T)
    traj, first_path = _launch(v, pol, rows, record=record, **kw)
    assert (traj is not None) == record
    out = _joined([traj]) if record else {}
    out.update(first_path=first_path, state=v.state, ts=v.ts)
    return out


# -- rl_rollout_gridworld_gru ---------------------------------------------------------------------------------------------
def _grid(desc="4x4", hidden=32, include_action=True, inject=True, cut=None):
    env, pol = _grid_policy(desc, hidden, state_include_action=include_action)
    ve = env.vec_env_executor(N, GRID_MPL, seed=3)
    u = _uniforms(T, N) if inject else None
    if cut is None:
        out = _joined([ve.rollout(pol, T, u=u)])
    else:
        out = _joined([ve.rollout(pol, cut, u=u[:cut]), ve.rollout(pol, T - cut, reset_at_start=False, u=u[cut:])])
    out["prob_out"] = out.pop("means")
    out.update(state=ve.state, ts=ve.ts, hidden_state=ve.hidden_state, prev_action=ve.prev_action)
    return out


CASES = {}
for _kind in (0, 2, 3):
    for _h in (32, 20, 64):
        CASES["gru_kind%d_h%d" % (_kind, _h)] = (_gru, dict(kind=_kind, hidden=_h))
    for _h in (32, 64):
        CASES["population_kind%d_h%d" % (_kind, _h)] = (_population, dict(kind=_kind, hidden=(_h, _h)))
CASES.update({
    "gru_kind2_h32_no_action": (_gru, dict(kind=2, include_action=False)),
    "gru_env_noise": (_gru, dict(cfg=NOISY)),
    "gru_continuation_12_13": (_gru, dict(cut=12)),
    "gru_philox": (_gru, dict(inject=False, seed=9)),
    "population_one_hidden_layer": (_population, dict(kind=2, hidden=(20,))),
    "population_env_noise": (_population, dict(cfg=NOISY)),
    "population_record_off": (_population, dict(record=False)),
    "population_philox": (_population, dict(inject=False, seed=9)),
    "grid_continuation_12_13": (_grid, dict(cut=12)),
    "grid_philox": (_grid, dict(inject=False)),
})
for _desc in ("4x4", "8x8"):
    for _h in (32, 64):
        for _ia in (0, 1):
            CASES["grid_%s_h%d_action%d" % (_desc, _h, _ia)] = (_grid, dict(desc=_desc, hidden=_h, include_action=bool(_ia)))


def run_case(name):
    """{array name: dict(shape, dtype, sha256)} of one case, on the current device."""
    fn, kw = CASES[name]
    torch.cuda.synchronize()
    out = {}
    for k, t in fn(**kw).items():
        a = np.ascontiguousarray(t.cpu().numpy())
        assert k != "dones" or a.sum() > a.shape[-1], "%s: every env is to end paths inside the launch" % name
        out[k] = dict(shape=list(a.shape), dtype=str(a.dtype), sha256=hashlib.sha256(a.tobytes()).hexdigest())
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["parent_commit"]) == 40 and sorted(g["cases"]) == sorted(CASES)
    return g["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_rollout_bits(name, golden):
    got, want = run_case(name), golden[name]
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], "%s: array %r differs from the recorded launch" % (name, k)
