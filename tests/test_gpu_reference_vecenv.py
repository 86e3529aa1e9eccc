"""HipVecEnv.step, NormalizingVecEnv (NormalizedEnv's running observation / reward normalisation on the vectorised
path) and the fused rollout's in-kernel normaliser against the reference's OWN code run here: its ``VecEnvExecutor``
(sandbox/rocky/tf/envs/vec_env_executor.py:8-33) over n of its ``NormalizedEnv`` copies
(rllab/envs/normalized_env.py:33-92), unmodified from the staged tree, driven with the recorded actions and the same
table of reset draws (oracle/ref_vecenv.py; the dynamics under the wrapper are the host float32 build, which the GPU
matches bit for bit -- tests/test_gpu_env_parity.py).  No restatement of the normaliser or of the lock-step rules lives
in this file.

Tolerances.  Gridded actions (tests/test_ref_vecenv.py::grid_actions) make NormalizedEnv's action map exact, so the raw
stream is bit-identical and: plain executor -> observations / rewards / dones compared BIT FOR BIT; running
normalisation -> the float64 estimates within 1e-12 (relative), the whitened float32 outputs within 2e-6.  Actions
sampled by the policy inside the fused rollout are not on the grid: the reference evaluates the map in numpy, the step
kernel with a fused multiply-add, one rounding of the scaled action apart -- 5e-5 (5e-4 on the contact-stiff two-legged
envs) relative to max(1, |x|).
"""
import importlib
import os

import numpy as np
import pytest
import torch

from test_ref_vecenv import draws_for, grid_actions, needs_ref

pytestmark = [pytest.mark.gpu, needs_ref]

ENVS = dict(cartpole=("rllab.envs.box2d.cartpole_env", "CartpoleEnv"),
            swingup=("rllab.envs.box2d.cartpole_swingup_env", "CartpoleSwingupEnv"),
            double_pendulum=("rllab.envs.box2d.double_pendulum_env", "DoublePendulumEnv"),
            swimmer=("rllab.envs.mujoco.swimmer_env", "SwimmerEnv"),
            cheetah=("rllab.envs.mujoco.half_cheetah_env", "HalfCheetahEnv"),
            walker=("rllab.envs.mujoco.walker2d_env", "Walker2DEnv"),
            hopper=("rllab.envs.mujoco.hopper_env", "HopperEnv"),
            idp=("rllab.envs.mujoco.inverted_double_pendulum_env", "InvertedDoublePendulumEnv"))


def make_env(name, **norm_kwargs):
    from rllab.envs.normalized_env import normalize
    mod, cls = ENVS[name]
    return normalize(getattr(importlib.import_module(mod), cls)(), **norm_kwargs)


def close(got, want, tol):
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))
    return float(err.max()) <= tol, float(err.max())


@pytest.mark.parametrize("name,mpl", [("cartpole", 9), ("cartpole", 0), ("swingup", 10), ("double_pendulum", 7), ("swimmer", 5),
                                      ("cheetah", 6), ("walker", 11), ("hopper", 12), ("idp", 8)])
def test_hipvecenv_step_is_the_reference_executor_bit_for_bit(name, mpl):
    """rl_vecenv_step's contract -- ts += 1, done |= ts >= max_path_length, a done copy reset inside the call and its
    RESET observation returned, NormalizedEnv's action map and scale_reward -- against the reference's executor."""
    from oracle import ref_vecenv
    env = make_env(name, scale_reward=0.25)
    n, T = 37, 40
    v = env.vec_env_executor(n_envs=n, max_path_length=mpl, seed=4)
    q = v.q
    rng = np.random.RandomState(5)
    draws = draws_for(q, rng, T, n)
    actions = grid_actions(rng, T, n, q["act_dim"])
    ref = ref_vecenv.run(v.kind, mpl, actions, draws, scale_reward=0.25)
    o = v.reset(draws=draws[0])
    assert np.array_equal(o.cpu().numpy().astype(np.float64), ref["obs"][0])
    n_done = 0
    for t in range(T):
        o, r, d, _ = v.step(torch.as_tensor(actions[t], device="cuda"), reset_draws=draws[t + 1])
        assert np.array_equal(d.cpu().numpy(), ref["dones"][t]), t
        assert np.array_equal(o.cpu().numpy().astype(np.float64), ref["obs"][t + 1]), t
        assert np.array_equal(r.cpu().numpy().astype(np.float64), ref["rewards"][t]), t
        n_done += int(d.sum())
    assert n_done >= (n if (mpl or v.terminates) else 0)


@pytest.mark.parametrize("name,flags,mpl", [("cartpole", (True, True), 15), ("cartpole", (False, True), 15),
                                            ("swimmer", (True, False), 6), ("cheetah", (True, True), 7),
                                            ("walker", (True, True), 12)])
def test_normalizing_vecenv_is_the_reference_normalized_env_per_copy(name, flags, mpl):
    """reset() / step() of the vectorised NormalizedEnv(normalize_obs / normalize_reward): per env copy the estimates
    are fed by every observation the copy produces, the TERMINAL one included, and once more by the reset observation,
    which is the one returned whitened; the reward is normalised, then scaled -- all as the reference's classes do it,
    starting from estimates that are not the initial 0 / 1 (a resumed snapshot)."""
    from oracle import ref_vecenv
    nobs, nrew = flags
    oa, ra, scale = 0.01, 0.02, 0.25
    env = make_env(name, scale_reward=scale, normalize_obs=nobs, normalize_reward=nrew, obs_alpha=oa, reward_alpha=ra)
    assert env.vectorized
    n, T = 33, 40
    v = env.vec_env_executor(n_envs=n, max_path_length=mpl, seed=4)
    q = v.q
    do = q["obs_dim"]
    rng = np.random.RandomState(0)
    draws = draws_for(q, rng, T, n)
    actions = grid_actions(rng, T, n, q["act_dim"])
    v.obs_mean += torch.as_tensor(0.1 * rng.randn(do, n), device=v.obs_mean.device)
    v.obs_var *= torch.as_tensor(1.0 + 0.5 * rng.rand(do, n), device=v.obs_var.device)
    v.reward_mean += 0.05
    v.reward_var *= 1.5
    ref = ref_vecenv.run(v.kind, mpl, actions, draws, scale_reward=scale, normalize_obs=nobs, normalize_reward=nrew,
                         obs_alpha=oa, reward_alpha=ra, obs_mean0=v.obs_mean.t().cpu().numpy(),
                         obs_var0=v.obs_var.t().cpu().numpy(), reward_mean0=v.reward_mean.cpu().numpy(),
                         reward_var0=v.reward_var.cpu().numpy())
    o = v.reset(draws=draws[0])
    ok, err = close(o.cpu().numpy(), ref["obs"][0], 2e-6)
    assert ok, err
    n_done = 0
    for t in range(T):
        o, r, d, _ = v.step(torch.as_tensor(actions[t], device="cuda"), reset_draws=draws[t + 1])
        assert np.array_equal(d.cpu().numpy(), ref["dones"][t]), t
        ok, err = close(o.cpu().numpy(), ref["obs"][t + 1], 2e-6)
        assert ok, (t, err)
        ok, err = close(r.cpu().numpy(), ref["rewards"][t], 2e-6)
        assert ok, (t, err)
        n_done += int(d.sum())
    assert n_done >= n                                       # terminal observations were part of the stream
    if nobs:
        np.testing.assert_allclose(v.obs_mean.t().cpu().numpy(), ref["obs_mean"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(v.obs_var.t().cpu().numpy(), ref["obs_var"], rtol=1e-12, atol=1e-14)
    if nrew:
        np.testing.assert_allclose(v.reward_mean.cpu().numpy(), ref["reward_mean"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(v.reward_var.cpu().numpy(), ref["reward_var"], rtol=1e-12, atol=1e-14)
    # the estimates travel with the env: pickling it (what every snapshot does) takes env copy 0's, and an executor
    # made from the unpickled env resumes from them instead of mean 0 / var 1
    import pickle
    clone = pickle.loads(pickle.dumps(env))
    if nobs:
        np.testing.assert_allclose(clone._obs_stats.mean, ref["obs_mean"][0], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(clone._obs_stats.var, ref["obs_var"][0], rtol=1e-12, atol=1e-14)
        v2 = clone.vec_env_executor(n_envs=3, max_path_length=mpl, seed=4)
        np.testing.assert_allclose(v2.obs_mean.cpu().numpy(), np.tile(ref["obs_mean"][0][:, None], (1, 3)), rtol=1e-12,
                                   atol=1e-14)


FUSED = [("cartpole", (True, True)), ("cartpole", (False, True)), ("cartpole", (False, False)), ("swimmer", (True, False)),
         ("cheetah", (True, True)), ("hopper", (True, True))]


def _fused_setup(name, flags, epw, monkeypatch, T, n=37, mpl=9):
    from rllab.policies.gaussian_mlp_policy import GaussianMLPPolicy
    monkeypatch.setenv("RLLAB_ROLLOUT_EPW", epw)
    nobs, nrew = flags
    kw = dict(scale_reward=0.25)
    if nobs or nrew:
        kw.update(normalize_obs=nobs, normalize_reward=nrew, obs_alpha=0.01, reward_alpha=0.02)
    env = make_env(name, **kw)
    np.random.seed(3)
    pol = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    v = env.vec_env_executor(n_envs=n, max_path_length=mpl, seed=6)
    assert v.takes_rollout_of(pol)
    plan = v.rollout_plan(pol, T)
    assert plan.kernel == 1 and plan.envs_per_wavefront == int(epw)
    assert (b"norm" in plan.name) == bool(nobs or nrew)
    q = v.q
    rng = np.random.RandomState(1)
    eps = rng.randn(q["act_dim"], T, n).astype(np.float32)
    draws = draws_for(q, rng, T, n)
    est0 = None
    if nobs or nrew:
        # a pre-existing estimate (a resumed snapshot): the kernel must start from it, not from mean 0 / var 1
        v.obs_mean += torch.as_tensor(0.1 * rng.randn(q["obs_dim"], n), device=v.obs_mean.device)
        v.reward_var *= 1.5
        est0 = dict(obs_mean0=v.obs_mean.t().cpu().numpy(), obs_var0=v.obs_var.t().cpu().numpy(),
                    reward_mean0=v.reward_mean.cpu().numpy(), reward_var0=v.reward_var.cpu().numpy(),
                    normalize_obs=nobs, normalize_reward=nrew, obs_alpha=0.01, reward_alpha=0.02)
    return env, pol, v, eps, draws, est0


def _check_fused_against_reference(name, v, traj, draws, est0, mpl, min_dones=None, before=None):
    """``min_dones``: how many paths the batch must at least end (default: one per env).  ``before`` (actions [T0, n, Da],
    draws [T0 + 1, R, n]): the executor sampled that batch from ``est0`` first and ``traj`` after a reset of its own; the
    reference's executor does the same on the same env copies (a Box2D world keeps its warm-start impulses over a reset)
    and is compared from that reset on."""
    from oracle import ref_vecenv
    tol = 5e-4 if name in ("cheetah", "walker", "hopper") else 5e-5
    T, n = traj.T, traj.N
    actions = traj.actions.permute(1, 2, 0).cpu().numpy()                     # [T, n, Da] as the policy sampled them
    if before is None:
        ref = ref_vecenv.run(v.kind, mpl, actions, draws, scale_reward=0.25, **(est0 or {}))
    else:
        T0 = before[0].shape[0]
        ref = ref_vecenv.run(v.kind, mpl, np.concatenate([before[0], actions]), np.concatenate([before[1], draws]),
                             scale_reward=0.25, reset_at=[T0], **(est0 or {}))
        ref.update(dones=ref["dones"][T0:], rewards=ref["rewards"][T0:], obs=ref["obs"][T0:])
    assert np.array_equal(traj.dones.cpu().numpy().astype(bool), ref["dones"])
    ok, err = close(traj.obs.permute(1, 2, 0).cpu().numpy(), ref["obs"][:T], tol)   # obs[t]: what action t was computed from
    assert ok, err
    ok, err = close(traj.rewards.cpu().numpy(), ref["rewards"], tol)
    assert ok, err
    ok, err = close(v._obs.t().cpu().numpy(), ref["obs"][T], tol)              # and the one the NEXT launch carries on from
    assert ok, err
    if est0 is not None and est0["normalize_obs"]:
        ok, err = close(v.obs_mean.t().cpu().numpy(), ref["obs_mean"], tol)
        assert ok, err
        ok, err = close(v.obs_var.t().cpu().numpy(), ref["obs_var"], tol)
        assert ok, err
    if est0 is not None and est0["normalize_reward"]:
        ok, err = close(v.reward_mean.cpu().numpy(), ref["reward_mean"], tol)
        assert ok, err
        ok, err = close(v.reward_var.cpu().numpy(), ref["reward_var"], tol)
        assert ok, err
    assert int(ref["dones"].sum()) >= (n if min_dones is None else min_dones)
    return ref


@pytest.mark.parametrize("name,flags", FUSED)
@pytest.mark.parametrize("epw", ["16", "64"])
def test_fused_rollout_is_the_reference_executor_on_its_own_actions(name, flags, epw, monkeypatch, quiet_logger):
    """The whole horizon in ONE launch -- with the wrapper's per-env running estimates inside the kernel when
    normalize_obs / normalize_reward -- against the reference's executor + NormalizedEnv copies stepping through the
    actions the launch recorded; policy means within 1e-5 of a float64 forward of the recorded observations."""
    T, mpl = 30, 9
    env, pol, v, eps, draws, est0 = _fused_setup(name, flags, epw, monkeypatch, T, mpl=mpl)
    traj = v.rollout(pol, T, eps=eps, reset_draws=draws)
    _check_fused_against_reference(name, v, traj, draws, est0, mpl)
    do, da = v.q["obs_dim"], v.q["act_dim"]
    with torch.no_grad():
        mean64 = pol.mean_planes(traj.obs.reshape(do, -1).double(), pol.flat_params.double())
    assert float((traj.means.reshape(da, -1).double() - mean64).abs().max()) <= 1e-5


@pytest.mark.parametrize("name,flags", [("cartpole", (True, True)), ("cartpole", (False, False)), ("hopper", (True, True))])
def test_fused_rollout_carried_on_without_a_reset_is_one_stream(name, flags, monkeypatch, quiet_logger):
    """Two launches, the second with reset_at_start=False (what the sampler does until batch_size whole-path samples
    are in): the envs carry on from their state, step count, estimates and the observation the first launch ended on --
    the joined batch is ONE run of the reference's executor, nothing reset, drawn or fed twice at the seam."""
    from rllab_amd.sampler.trajectories import Trajectories
    T1, T2, mpl = 13, 17, 9
    T = T1 + T2
    env, pol, v, eps, draws, est0 = _fused_setup(name, flags, "16", monkeypatch, T, mpl=mpl)
    a = v.rollout(pol, T1, eps=eps[:, :T1].copy(), reset_draws=draws[:T1 + 1].copy())
    b = v.rollout(pol, T2, reset_at_start=False, eps=eps[:, T1:].copy(), reset_draws=draws[T1:].copy())
    traj = Trajectories.concat([a, b])
    assert (traj.T, traj.N) == (T, 37)
    _check_fused_against_reference(name, v, traj, draws, est0, mpl)
