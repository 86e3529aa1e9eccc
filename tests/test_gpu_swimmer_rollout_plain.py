"""The Swimmer lane-group rollout has two instantiations of one body: the PLAIN one (in-kernel Philox policy noise and
reset draws, no action / observation noise, no injected planes -- what a training run launches) and the generic one
(every option tested at run time).  The launcher takes the plain one exactly when every left-out option is off.

* plain against the reference, bit for bit on every plane: the generic kernel, given as ``eps`` the very N(0,1) draws
  the plain kernel makes in-kernel, and the host build of the dynamics replaying the recorded actions.
  The draws are taken from the env-per-lane ``rollout_kernel`` (another kernel, the same Philox block per (seed, env,
  step)) under a policy of all-zero parameters: mean = 0 and std = exp(0) = 1, so the recorded action fma(z, 1, 0) IS z.
  The float transform of the draws uses hardware transcendentals and has no host restatement (csrc/device_rng.h), which
  is also why the reset draws stay in-kernel on both sides of the comparison; the host replay rebuilds each path's
  reset state from its first observation (oracle/replay.py).
* dispatch: with each left-out option on, the call takes the generic kernel and is the host build's result.
"""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWIMMER = 2
MPL = 4           # paths end inside a launch: resets, and the lane-group state handed over afresh (chain_valid = false)
SWITCHES = ("RLLAB_ROLLOUT_EPW", "RLLAB_ROLLOUT_WPB", "RLLAB_SWIMMER_LANE_KERNEL", "RLLAB_SWIMMER_COOP")


def _policy(hidden, nl="tanh", seed=0, zero=False):
    from rllab_amd import _lib
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    from rllab_amd.spaces import Box
    q = _lib.env_query(SWIMMER)
    np.random.seed(seed)
    spec = EnvSpec(Box(-1e6 * np.ones(q["obs_dim"]), 1e6 * np.ones(q["obs_dim"])),
                   Box(-np.ones(q["act_dim"]), np.ones(q["act_dim"])))
    pol = GaussianMLPPolicy(spec, hidden_sizes=hidden, hidden_nonlinearity=dict(tanh=torch.tanh, rectify=rectify)[nl])
    if zero:
        pol.flat_params.zero_()          # weights, biases and log_std: mean = 0, std = 1
    return pol


def _two_launches(policy, n, T, seed, eps=(None, None), cfg=None, **planes):
    """reset_at_start = 1, then a second launch that carries on; every plane of both, the final state, ts, last_obs"""
    from rllab_amd.envs.hip_env import HipVecEnv
    v = HipVecEnv(SWIMMER, n, MPL, normalize=True, scale_reward=0.5, seed=seed, env_offset=5, cfg=cfg)
    trs = [v.rollout(policy, T, reset_at_start=True, eps=eps[0], **{k: p[0] for k, p in planes.items()}),
           v.rollout(policy, T, reset_at_start=False, eps=eps[1], **{k: p[1] for k, p in planes.items()})]
    torch.cuda.synchronize()
    out = {k: torch.cat([getattr(tr, k) for tr in trs], dim=-2).cpu().numpy()
           for k in ("obs", "actions", "means", "rewards", "dones")}
    out.update(state=v.state.cpu().numpy(), ts=v.ts.cpu().numpy(), last_obs=v._obs.cpu().numpy())
    return v, out


def _joined(out, n):
    """the two launches as one trajectory for oracle.replay"""
    g = lambda k: torch.as_tensor(out[k])
    return types.SimpleNamespace(T=out["rewards"].shape[0], N=n, obs=g("obs"), actions=g("actions"),
                                 rewards=g("rewards"), dones=g("dones"))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _plan(v, policy, T):
    p = v.rollout_plan(policy, T)
    return int(p.kernel), p.name.decode() if isinstance(p.name, bytes) else str(p.name)


CASES = [(n, T, h, "tanh") for n in (16, 17, 48) for T in (3, 9) for h in (32, 64)] + [(17, 9, 32, "rectify")]


@pytest.mark.parametrize("n,T,h,nl", CASES)
def test_plain_kernel_is_the_generic_kernel_and_the_host_build(n, T, h, nl, monkeypatch):
    """n = 16: one wavefront; 17: a second one with one live lane; 48: three.  T = 9 crosses two of the four-step noise
    blocks.  Every plane, the final state, ts and last_obs: equal bit for bit."""
    from oracle.replay import replay_check
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    policy = _policy((h, h), nl)
    v, plain = _two_launches(policy, n, T, seed=31)
    assert _plan(v, policy, T)[0] == 4
    assert plain["dones"].sum() > 0 and plain["dones"].sum() < plain["dones"].size
    # the draws of the same (seed, env, step) from the env-per-lane kernel under the all-zero policy
    monkeypatch.setenv("RLLAB_SWIMMER_LANE_KERNEL", "1")
    monkeypatch.setenv("RLLAB_ROLLOUT_EPW", "64")
    zero = _policy((h, h), nl, zero=True)
    vz, drawn = _two_launches(zero, n, T, seed=31)
    assert _plan(vz, zero, T)[0] != 4
    monkeypatch.delenv("RLLAB_SWIMMER_LANE_KERNEL")
    monkeypatch.delenv("RLLAB_ROLLOUT_EPW")
    z = drawn["actions"]
    assert np.all(drawn["means"] == 0.0) and np.isfinite(z).all() and 0.5 < z.std() < 1.5
    # generic kernel, the same draws injected
    _, generic = _two_launches(policy, n, T, seed=31, eps=(z[:, :T].copy(), z[:, T:].copy()))
    for k in sorted(plain):
        bad = np.flatnonzero(_bits(plain[k]).reshape(-1) != _bits(generic[k]).reshape(-1))
        print("%s: %d of %d words differ" % (k, bad.size, plain[k].size))
        assert bad.size == 0, (k, bad[:8])
    # host build of the dynamics from the recorded actions, across the join of the two launches
    assert replay_check(v, _joined(plain, n), max_envs=n) == 2 * T * n


def _draws(rng, T, n):
    from rllab_amd import _lib
    q = _lib.env_query(SWIMMER)
    return [rng.randn(T + 1, q["reset_draws"], n).astype(np.float32) for _ in range(2)]


@pytest.mark.parametrize("option", ["eps", "action_noise", "obs_noise", "reset_draws"])
def test_each_left_out_option_takes_the_generic_kernel(option, monkeypatch):
    """Injected eps / action noise / observation noise / reset-draw planes: the launch succeeds under the same plan and
    is the host build's result for the same inputs (replayed with the planes the launch was given)."""
    from rllab_amd import _lib
    from oracle.replay import replay_check
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    q = _lib.env_query(SWIMMER)
    rng = np.random.RandomState(5)
    n, T = 17, 9
    policy = _policy((32, 32))
    kw, cfg, replay_kw = {}, None, {}
    eps = (None, None)
    if option == "eps":
        eps = tuple(rng.randn(q["act_dim"], T, n).astype(np.float32) for _ in range(2))
    elif option == "action_noise":
        cfg = dict(action_noise=0.1)
        kw["action_noise_z"] = [rng.randn(T, q["act_dim"], n).astype(np.float32) for _ in range(2)]
        replay_kw["action_noise_z"] = np.concatenate(kw["action_noise_z"], axis=0)
    elif option == "obs_noise":
        cfg = dict(obs_noise=0.05)
        kw["obs_noise_z"] = [rng.randn(T + 1, q["obs_dim"], n).astype(np.float32) for _ in range(2)]
        kw["reset_draws"] = _draws(rng, T, n)      # a noisy observation does not determine the reset state
    else:
        kw["reset_draws"] = _draws(rng, T, n)
    v, out = _two_launches(policy, n, T, seed=8, eps=eps, cfg=cfg, **kw)
    assert _plan(v, policy, T) == (4, "rollout_swimmer_quad_kernel<32>")
    assert out["dones"].sum() > 0 and np.isfinite(out["obs"]).all()
    if option == "eps":
        std = np.exp(policy.effective_log_std().cpu().numpy())[:, None, None]
        want = out["means"].astype(np.float64) + np.concatenate(eps, axis=1).astype(np.float64) * std
        assert np.abs(out["actions"] - want).max() <= 1e-6
    if "reset_draws" in kw:
        # slice T of the first launch is never used (the second launch carries on); slice t of the second launch resets
        # before its step t = joined step T + t
        a, b = kw["reset_draws"]
        replay_kw["reset_draws"] = np.concatenate([a[:T], b], axis=0)
    if "obs_noise_z" in kw:
        # the lane-group kernel observes its state afresh at the start of a launch: joined observation T carries slice 0
        # of the second launch (slice T of the first went to last_obs only)
        a, b = kw["obs_noise_z"]
        replay_kw["obs_noise_z"] = np.concatenate([a[:T], b], axis=0)
    assert replay_check(v, _joined(out, n), max_envs=n, **replay_kw) == 2 * T * n
