"""The fused deterministic rollout (rl_rollout_deterministic_mlp, HipVecEnv.rollout_deterministic): a DeterministicMLPPolicy
under OUStrategy / GaussianStrategy / no exploration, one env per lane.

N = 70 envs (a partial last wavefront), T = 25 lock-steps, paths cut at 11: resets and cuts happen inside the launch.
normalize=True; the strategy's draws and the reset draws are injected.  The env dynamics replay bit for bit on the host
build, the actions are bit-equal to the float32 restatement of the strategy's rule on the recorded means, the means are
measured against the float64 forward over the recorded observations."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_det_rollout_host import _forward64, _spec

pytestmark = pytest.mark.gpu

N, T, MPL = 70, 25, 11
NETS = {"32x32": ((32, 32), "rectify", "tanh"), "20x7": ((20, 7), "tanh", None), "64x64": ((64, 64), "rectify", "tanh")}
OU = dict(mu=0.0, theta=0.15, sigma=0.3)
SEED = 5


def _policy(kind, net, seed=0):
    """A policy of NETS[net] on env ``kind`` with every block non-trivial: the reference's hidden weights, biases in
    +-0.1, output weights in +-0.05 (|mean| of a few tenths: the strategy's noise clips some actions and not others)."""
    from rllab_amd import _lib
    from rllab_amd.core.network import rectify
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    hidden, hf, of = NETS[net]
    q = _lib.env_query(kind)
    np.random.seed(seed)
    pol = DeterministicMLPPolicy(_spec(q["obs_dim"], q["act_dim"]), hidden_sizes=hidden,
                                 hidden_nonlinearity=rectify if hf == "rectify" else torch.tanh,
                                 output_nonlinearity=torch.tanh if of == "tanh" else None)
    rng = np.random.RandomState(seed + 1)
    flat = pol.get_param_values()
    D, (h0, h1), A = q["obs_dim"], hidden, q["act_dim"]
    b0, w1, b1, w2 = D * h0, D * h0 + h0, D * h0 + h0 + h0 * h1, D * h0 + h0 + h0 * h1 + h1
    flat[b0:w1] = rng.uniform(-0.1, 0.1, h0)
    flat[b1:w2] = rng.uniform(-0.1, 0.1, h1)
    flat[w2:] = rng.uniform(-0.05, 0.05, h1 * A + A)
    pol.set_param_values(flat)
    return pol


def _noise(q, n, horizon, seed=1):
    rng = np.random.RandomState(seed)
    eps = rng.randn(q["act_dim"], horizon, n).astype(np.float32)
    draws = (rng.randn if q["reset_is_normal"] else rng.rand)(horizon + 1, q["reset_draws"], n).astype(np.float32)
    return eps, draws


def _np(t):
    return t.cpu().numpy()


def ou_actions(eps, means, dones, low, high, mu, theta, sigma, x=None):
    """The float32 recurrence of OUStrategy.evolve_states / get_actions / reset(mask) on planes [A, T, n]: every
    operation rounded once.  Returns (actions, the state x after the last step)."""
    f = np.float32
    A, steps, n = means.shape
    x = np.full((A, n), mu, dtype=f) if x is None else x.astype(f).copy()
    act = np.empty_like(means)
    for t in range(steps):
        x = x + (f(theta) * (f(mu) - x) + f(sigma) * eps[:, t])
        assert x.dtype == f
        act[:, t] = np.maximum(np.minimum(means[:, t] + x, high[:, None]), low[:, None])
        x[:, dones[t] != 0] = f(mu)
    return act, x


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@functools.lru_cache(maxsize=None)
def _ou_run(kind, net, n=N):
    """One launch under the OU rule, shared by the tests that read it (nothing here is written afterwards)."""
    from rllab_amd.envs.hip_env import HipVecEnv
    from rllab_amd.exploration_strategies.ou_strategy import OUStrategy
    pol = _policy(kind, net)
    v = HipVecEnv(kind, n, MPL, normalize=True, seed=SEED)
    es = OUStrategy(pol.env_spec, **OU)
    eps, draws = _noise(v.q, n, T)
    traj = v.rollout_deterministic(pol, T, es=es, eps=eps, reset_draws=draws)
    torch.cuda.synchronize()
    return pol, v, es, eps, draws, traj


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("kind", [0, 2, 3])
def test_parity(kind, net):
    from oracle.replay import replay_check
    pol, v, es, eps, draws, traj = _ou_run(kind, net)
    q = v.q
    assert v.step_counter == T + 1
    assert replay_check(v, traj, max_envs=N, reset_draws=draws) == N * T
    means, act, dones = _np(traj.means), _np(traj.actions), _np(traj.dones)
    low, high = -np.ones(q["act_dim"], np.float32), np.ones(q["act_dim"], np.float32)
    want, x = ou_actions(eps, means, dones, low, high, **OU)
    clipped = float(np.mean(np.abs(want) == 1.0))
    print("kind %d net %s: share of clipped actions %.3f, max |mean| %.3f" % (kind, net, clipped, np.abs(means).max()))
    assert 0.0 < clipped < 1.0
    assert np.array_equal(_bits(act), _bits(want))
    assert tuple(es.states.shape) == (N, q["act_dim"]) and np.array_equal(_bits(_np(es.states).T), _bits(x))
    # the means: against the float64 forward over the recorded observations.  The yardstick is the float32 forward of
    # torch on the CPU on the same observations -- both are float32 sums of the same length in different orders, hence
    # 4 x its own worst deviation -- with a floor of 2^-22 (4 ulp of a tanh output; for the identity output the same
    # relative to the largest mean, at least 1).
    hidden, hf, of = NETS[net]
    obs = _np(traj.obs).reshape(q["obs_dim"], -1).T
    flat = pol.get_param_values()
    m64 = _forward64(flat, q["obs_dim"], hidden[0], hidden[1], q["act_dim"], hf, of, obs.astype(np.float64))
    with torch.no_grad():
        m32 = pol.action_planes(torch.as_tensor(obs.T.copy()), torch.as_tensor(flat, dtype=torch.float32)).numpy().T
    got = means.reshape(q["act_dim"], -1).T
    err_gpu, err_cpu = float(np.abs(got - m64).max()), float(np.abs(m32.astype(np.float64) - m64).max())
    floor = 2.0 ** -22 * (1.0 if of == "tanh" else max(1.0, float(np.abs(m64).max())))
    print("kind %d net %s: means vs float64: kernel %.3e, float32 torch on the CPU %.3e (bound %.3e)" % (
        kind, net, err_gpu, err_cpu, max(4.0 * err_cpu, floor)))
    assert err_gpu <= max(4.0 * err_cpu, floor)
    assert np.array_equal(_np(traj.log_std), np.full(q["act_dim"], -np.inf, np.float32))


@pytest.mark.parametrize("kind", [0, 2])
def test_cuts_are_the_paths_the_env_did_not_end(kind):
    """Recount with the host env, stepped on the recorded actions as oracle/replay.py steps it."""
    from oracle import host_env as H
    pol, v, es, eps, draws, traj = _ou_run(kind, "32x32")
    act, dones, cuts = _np(traj.actions), _np(traj.dones).astype(bool), _np(traj.cuts).astype(bool)
    host_done = np.zeros((T, N), dtype=bool)
    path_step = np.zeros((T, N), dtype=np.int64)
    for n in range(N):
        env = H.HostEnv(kind, np.float32, normalize=True)
        fresh, ts = True, 0
        for t in range(T):
            if fresh:
                env.reset(draws[t, :, n])
                fresh, ts = False, 0
            _, _, d = env.step(act[:, t, n])
            ts += 1
            host_done[t, n], path_step[t, n] = bool(d), ts
            fresh = bool(d) or ts >= MPL
    assert np.array_equal(dones, host_done | (path_step >= MPL))
    assert np.array_equal(cuts, dones & ~host_done)
    assert np.all(path_step[cuts] == MPL)
    print("kind %d: paths ended by the env %d, cut at the horizon %d" % (kind, host_done.sum(), cuts.sum()))
    assert cuts.sum() > 0
    if kind == 0:
        assert host_done.sum() > 0


def test_gaussian_strategy():
    """decay_period = 15 lock-steps: sigma_t changes every step and sits on min_sigma from t = 15 on."""
    from rllab_amd.envs.hip_env import HipVecEnv
    from rllab_amd.exploration_strategies.gaussian_strategy import GaussianStrategy
    kind = 2
    pol = _policy(kind, "32x32")
    v = HipVecEnv(kind, N, MPL, normalize=True, seed=SEED)
    es = GaussianStrategy(pol.env_spec, max_sigma=1.0, min_sigma=0.1, decay_period=15 * N)
    eps, draws = _noise(v.q, N, T)
    itr = 2 * N
    traj = v.rollout_deterministic(pol, T, es=es, itr=itr, eps=eps, reset_draws=draws)
    sig = np.asarray([es.sigma(itr + t * N) for t in range(T)], dtype=np.float32)
    assert len(set(sig[:13].tolist())) == 13 and np.all(sig[13:] == np.float32(0.1))
    means = _np(traj.means)
    want = np.maximum(np.minimum(means + eps * sig[None, :, None], np.float32(1.0)), np.float32(-1.0))
    assert want.dtype == np.float32 and 0.0 < np.mean(np.abs(want) == 1.0) < 1.0
    assert np.array_equal(_bits(_np(traj.actions)), _bits(want))


def test_no_exploration():
    from oracle.replay import replay_check
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 0
    pol = _policy(kind, "20x7")
    v = HipVecEnv(kind, N, MPL, normalize=True, seed=SEED)
    _, draws = _noise(v.q, N, T)
    traj = v.rollout_deterministic(pol, T, reset_draws=draws)
    assert replay_check(v, traj, max_envs=N, reset_draws=draws) == N * T
    assert np.array_equal(_bits(_np(traj.actions)), _bits(_np(traj.means))) and np.abs(_np(traj.means)).max() > 0
    assert np.array_equal(_np(traj.log_std), np.asarray([-np.inf], np.float32))
    assert int(traj.cuts.sum()) > 0


@pytest.mark.parametrize("kind", [0, 2])
def test_carry_on(kind):
    """25 lock-steps in one launch and as 10 + 15, the second without a reset: every plane and every carried buffer."""
    from rllab_amd.envs.hip_env import HipVecEnv
    from rllab_amd.exploration_strategies.ou_strategy import OUStrategy
    pol, v, es, eps, draws, whole = _ou_run(kind, "32x32")
    v2 = HipVecEnv(kind, N, MPL, normalize=True, seed=SEED)
    es2 = OUStrategy(pol.env_spec, **OU)
    a = v2.rollout_deterministic(pol, 10, es=es2, eps=eps[:, :10].copy(), reset_draws=draws[:11].copy())
    b = v2.rollout_deterministic(pol, 15, es=es2, reset_at_start=False, eps=eps[:, 10:].copy(),
                                 reset_draws=draws[10:].copy())
    assert v2.step_counter == 11 + 16
    dones = _np(whole.dones)
    assert (dones[:10].sum(axis=0) == 0).any() and dones[10].any()      # paths that run across the cut, and end behind it
    for name in ("obs", "actions", "means"):
        got = torch.cat([getattr(a, name), getattr(b, name)], dim=1)
        assert np.array_equal(_bits(_np(got)), _bits(_np(getattr(whole, name)))), name
    for name in ("rewards", "dones", "cuts"):
        got = torch.cat([getattr(a, name), getattr(b, name)], dim=0)
        assert np.array_equal(_bits(_np(got)), _bits(_np(getattr(whole, name)))), name
    for name in ("state", "ts", "_obs"):
        assert np.array_equal(_bits(_np(getattr(v2, name))), _bits(_np(getattr(v, name)))), name
    assert np.array_equal(_bits(_np(es2.states)), _bits(_np(es.states))) and float(es.states.abs().max()) > 0


def test_philox_path():
    """No injected planes: the draws are the Philox streams at (seed, env, step counter)."""
    from rllab_amd.envs.hip_env import HipVecEnv
    from rllab_amd.exploration_strategies.ou_strategy import OUStrategy
    kind = 0
    pol = _policy(kind, "32x32")
    runs = []
    for _ in range(2):
        v = HipVecEnv(kind, N, MPL, normalize=True, seed=SEED)
        es = OUStrategy(pol.env_spec, **OU)
        runs.append([v.rollout_deterministic(pol, T, es=es), v.rollout_deterministic(pol, T, es=es)])
    planes = ("obs", "actions", "means", "rewards", "dones", "cuts")
    for name in planes:
        assert np.array_equal(_bits(_np(getattr(runs[0][0], name))), _bits(_np(getattr(runs[1][0], name)))), name
        assert np.array_equal(_bits(_np(getattr(runs[0][1], name))), _bits(_np(getattr(runs[1][1], name)))), name
    first, second = runs[0]
    assert not np.array_equal(_np(first.actions), _np(second.actions))
    assert not np.array_equal(_np(first.obs[:, 0]), _np(second.obs[:, 0]))          # other reset draws
    # the exploration is there: actions differ from the means, within the bounds
    assert not np.array_equal(_np(first.actions), _np(first.means)) and float(first.actions.abs().max()) <= 1.0


def test_one_env():
    from oracle.replay import replay_check
    pol, v, es, eps, draws, traj = _ou_run(0, "32x32", 1)
    assert replay_check(v, traj, max_envs=1, reset_draws=draws) == T
    want, x = ou_actions(eps, _np(traj.means), _np(traj.dones), -np.ones(1, np.float32), np.ones(1, np.float32), **OU)
    assert np.array_equal(_bits(_np(traj.actions)), _bits(want)) and np.array_equal(_bits(_np(es.states).T), _bits(x))
    assert int(traj.dones.sum()) >= 2


def test_argument_errors_launch_nothing():
    from rllab_amd import _lib
    kind, n, horizon = 3, N, 5
    q = _lib.env_query(kind)
    pol = _policy(kind, "32x32")
    theta, (h0, h1), (hf, of) = pol.rollout_layout()
    dev = theta.device
    sevens = lambda shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=dev)
    buf = dict(state=sevens((q["state_dim"], n)), ts=sevens((n,), torch.int32), last_obs=sevens((q["obs_dim"], n)),
               explore_state=sevens((q["act_dim"], n)), obs=sevens((q["obs_dim"], horizon, n)),
               actions=sevens((q["act_dim"], horizon, n)), means=sevens((q["act_dim"], horizon, n)),
               rewards=sevens((horizon, n)), dones=sevens((horizon, n), torch.uint8),
               cuts=sevens((horizon, n), torch.uint8))
    sigma_t = sevens((horizon,))
    bounds = (ctypes.c_float * q["act_dim"])(*([1.0] * q["act_dim"]))

    def call(**kw):
        a = _lib.DetRolloutArgs(kind=kind, n_envs=n, horizon=horizon, max_path_length=MPL, normalize=1, reset_at_start=1,
                                hidden0=h0, hidden1=h1, hidden_activation=hf, output_activation=of,
                                explore=_lib.EXPLORE_OU, scale_reward=1.0, ou_theta=0.15, ou_sigma=0.3, seed=SEED,
                                theta=theta.data_ptr(), sigma_t=sigma_t.data_ptr(), low=bounds, high=bounds)
        for name, t in buf.items():
            setattr(a, name, t.data_ptr())
        for k, val in kw.items():
            setattr(a, k, val)
        rc = _lib.lib.rl_rollout_deterministic_mlp(ctypes.byref(a), _lib.stream_ptr())
        return rc, _lib.lib.rl_last_error()

    bad = [dict(n_envs=0), dict(horizon=0), dict(theta=None), dict(hidden0=0), dict(hidden0=65), dict(hidden1=30),
           dict(hidden1=68), dict(explore=3), dict(low=None), dict(high=None), dict(explore_state=None),
           dict(explore=_lib.EXPLORE_GAUSSIAN, sigma_t=None), dict(kind=99)]
    bad += [{name: None} for name in buf if name not in ("cuts", "explore_state")]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1, (kw, rc, msg)
    cfg = _lib.env_default_cfg(kind, flags=_lib.CFG_CONTACT_MUJOCO)
    rc, msg = call(cfg=ctypes.pointer(cfg))
    assert rc == -2 and b"soft-constraint" in msg, (rc, msg)
    torch.cuda.synchronize()
    for name, t in buf.items():
        assert bool((t == 7).all()), name
    buf["state"].zero_()
    buf["ts"].zero_()
    rc, msg = call()                                                     # and the same block as it stands is taken
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not bool((buf["obs"] == 7).all()) and int(buf["ts"].max()) <= MPL
