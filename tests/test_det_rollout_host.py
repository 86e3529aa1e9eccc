"""The fused deterministic rollout without a device: the padded parameter layout of a DeterministicMLPPolicy, the rule
the exploration strategies hand the kernel, the update count of a chunk against the lock-step loop's, the path returns
recounted from a chunk's planes, the new refusals and the argument checks of rl_rollout_deterministic_mlp."""
import ctypes

import numpy as np
import pytest
import torch


def _spec(D, A):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Box
    return EnvSpec(Box(-1e6 * np.ones(D), 1e6 * np.ones(D)), Box(-np.ones(A), np.ones(A)))


def _forward64(theta, D, H0, H1, A, hidden, out, obs):
    """float64 forward of the kernel's flat layout W0[D][H0] b0 W1[H0][H1] b1 W2[H1][A] b2 on obs [B, D]."""
    th = np.asarray(theta, dtype=np.float64)
    cut = np.cumsum([D * H0, H0, H0 * H1, H1, H1 * A, A])
    W0, b0, W1, b1, W2, b2 = np.split(th, cut[:-1])
    f = {"rectify": lambda x: np.maximum(x, 0.0), "tanh": np.tanh, None: lambda x: x}
    h = f[hidden](obs @ W0.reshape(D, H0) + b0)
    h = f[hidden](h @ W1.reshape(H0, H1) + b1)
    return f[out](h @ W2.reshape(H1, A) + b2)


def test_layout_pads_with_zeros_and_keeps_the_function():
    from rllab_amd import _lib
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    np.random.seed(0)
    D, A = 13, 2
    pol = DeterministicMLPPolicy(_spec(D, A), hidden_sizes=(20, 7), hidden_nonlinearity=torch.tanh,
                                 output_nonlinearity=None)
    flat = pol.get_param_values()
    flat[13 * 20:13 * 20 + 20] = np.random.uniform(-0.1, 0.1, 20)           # the reference starts the biases at zero
    flat[13 * 20 + 20 + 20 * 7:13 * 20 + 20 + 20 * 7 + 7] = np.random.uniform(-0.1, 0.1, 7)
    pol.set_param_values(flat)
    theta, (H0, H1), codes = pol.rollout_layout()
    assert (H0, H1) == (20, 8) and codes == (_lib.ACT_TANH, _lib.ACT_IDENTITY)
    assert theta.dtype == torch.float32 and theta.numel() == D * 20 + 20 + 20 * 8 + 8 + 8 * A + A
    th = theta.numpy()
    W1 = th[D * 20 + 20:D * 20 + 20 + 20 * 8].reshape(20, 8)
    b1 = th[D * 20 + 20 + 20 * 8:D * 20 + 20 + 20 * 8 + 8]
    W2 = th[D * 20 + 20 + 20 * 8 + 8:D * 20 + 20 + 20 * 8 + 8 + 8 * A].reshape(8, A)
    assert not W1[:, 7].any() and b1[7] == 0 and not W2[7].any()               # the padding unit
    assert np.count_nonzero(th) == np.count_nonzero(pol.get_param_values())
    obs = np.random.RandomState(1).randn(50, D)
    padded = _forward64(th, D, 20, 8, A, "tanh", None, obs)
    plain = _forward64(pol.get_param_values(), D, 20, 7, A, "tanh", None, obs)
    assert np.array_equal(padded, plain)
    assert np.allclose(plain, pol.get_actions(torch.as_tensor(obs, dtype=torch.float32))[0].numpy(), atol=1e-5)
    # the layout follows the parameters as they are now
    pol.set_param_values(pol.get_param_values() * 2.0)
    assert np.array_equal(pol.rollout_layout()[0].numpy(), 2.0 * th)
    # multiples of 4 stay as they are; every width 1 .. 64 is taken
    assert DeterministicMLPPolicy(_spec(4, 1)).rollout_layout()[1] == (32, 32)
    assert DeterministicMLPPolicy(_spec(4, 1), hidden_sizes=(1, 61)).rollout_layout()[1] == (4, 64)


def test_layout_refusals():
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    spec = _spec(4, 1)
    for kw, word in ((dict(hidden_sizes=(128, 32)), "1 .. 64"), (dict(hidden_sizes=(32,)), "two hidden layers"),
                     (dict(hidden_nonlinearity=torch.sigmoid), "rectify or tanh"),
                     (dict(hidden_nonlinearity=None), "identity"),
                     (dict(output_nonlinearity=torch.relu), "tanh or the identity")):
        pol = DeterministicMLPPolicy(spec, **kw)
        assert word in pol.why_no_rollout_layout(), (kw, pol.why_no_rollout_layout())
        with pytest.raises(NotImplementedError, match=word):
            pol.rollout_layout()
    assert "32 observation" in DeterministicMLPPolicy(_spec(33, 1)).why_no_rollout_layout()
    assert "8 action" in DeterministicMLPPolicy(_spec(4, 9)).why_no_rollout_layout()


def test_strategies_hand_over_their_rule():
    from rllab_amd import _lib
    from rllab_amd.exploration_strategies.gaussian_strategy import GaussianStrategy
    from rllab_amd.exploration_strategies.ou_strategy import OUStrategy
    from rllab_amd.spaces import Box
    from rllab_amd.envs.env_spec import EnvSpec
    spec = EnvSpec(Box(-np.ones(3), np.ones(3)), Box(np.array([-1.0, -0.5]), np.array([2.0, 0.25])))
    ou = OUStrategy(spec, mu=0.1, theta=0.2, sigma=0.4).kernel_rule(17, 5, 8, "cpu")
    assert ou["code"] == _lib.EXPLORE_OU and (ou["theta"], ou["mu"], ou["sigma"]) == (0.2, 0.1, 0.4)
    assert ou["low"].dtype == np.float32 and ou["low"].tolist() == [-1.0, -0.5] and ou["high"].tolist() == [2.0, 0.25]
    assert ou["sigma_t"] is None
    es = GaussianStrategy(spec, max_sigma=1.0, min_sigma=0.1, decay_period=100)
    g = es.kernel_rule(40, 6, 8, "cpu")                                  # itr = 40, 48, 56, ... : the floor from t = 8
    assert g["code"] == _lib.EXPLORE_GAUSSIAN and g["sigma_t"].dtype == torch.float32
    want = np.asarray([es.sigma(40 + 8 * t) for t in range(6)], dtype=np.float32)
    assert np.array_equal(g["sigma_t"].numpy(), want) and want[0] == np.float32(0.64) and len(set(want.tolist())) == 6
    assert es.kernel_rule(96, 3, 8, "cpu")["sigma_t"].tolist() == [np.float32(es.sigma(96)), np.float32(0.1), np.float32(0.1)]


def test_chunk_update_count_is_the_lock_step_loops():
    from rllab_amd.algos.ddpg import chunk_update_count
    checked = 0
    for capacity in (7, 24, 40, 1000):
        for n in (1, 3, 8):
            for min_pool in (1, 5, 24, 25, 41):
                for S in (1, 2, 5, 13):
                    if S * n > capacity:
                        continue
                    for size in sorted({0, 1, min(n, capacity), min(23, capacity), min(24, capacity), capacity}):
                        loop, s = 0, size
                        for _ in range(S):                           # DDPG.train: pool.add, then `if pool.size >= ...`
                            s = min(s + n, capacity)
                            loop += int(s >= min_pool)
                        assert chunk_update_count(size, n, S, min_pool, capacity) == loop, (size, n, S, min_pool, capacity)
                        checked += 1
    assert checked > 500


def test_path_returns_from_a_chunk_match_the_lock_step_loop():
    from rllab_amd.algos.ddpg import DDPG
    rng = np.random.RandomState(3)
    n, total = 5, 40
    rew = rng.randn(total, n).astype(np.float32)
    done = rng.rand(total, n) < 0.15
    done[:, 4] = False                                                   # one env never ends a path
    want = np.full((total, n), np.nan)
    run = np.zeros(n)
    for t in range(total):                                               # DDPG.train's bookkeeping
        run += rew[t].astype(np.float64)
        want[t, done[t]] = run[done[t]]
        run[done[t]] = 0.0
    carry = torch.zeros(n, dtype=torch.float64)
    got, t0 = [], 0
    for T in (1, 7, 1, 20, 11):
        got.append(DDPG._path_returns(torch.as_tensor(rew[t0:t0 + T]), torch.as_tensor(done[t0:t0 + T]).to(torch.uint8),
                                      carry).numpy())
        t0 += T
    got = np.concatenate(got)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isfinite(want).sum() > 10
    assert np.allclose(got[done], want[done], rtol=0, atol=1e-12)
    assert np.allclose(carry.numpy(), run, rtol=0, atol=1e-12)


class _Vectorized(object):
    """What DDPG's constructor reads of an env."""
    vectorized = True

    def __init__(self, D, A):
        self.spec = _spec(D, A)
        self.observation_space, self.action_space = self.spec.observation_space, self.spec.action_space


def test_ddpg_rollout_steps_refusals():
    from rllab_amd.algos.ddpg import DDPG
    from rllab_amd.exploration_strategies.base import ExplorationStrategy
    from rllab_amd.exploration_strategies.ou_strategy import OUStrategy
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab_amd.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    env = _Vectorized(4, 1)
    make = lambda **kw: DDPG(env=env, policy=DeterministicMLPPolicy(env.spec), qf=ContinuousMLPQFunction(env.spec),
                             es=kw.pop("es", OUStrategy(env.spec)), **kw)
    assert make().rollout_steps is None and make(rollout_steps=10).rollout_steps == 10
    with pytest.raises(TypeError):
        DDPG(env, DeterministicMLPPolicy(env.spec), ContinuousMLPQFunction(env.spec), OUStrategy(env.spec), 32, 200, 1000,
             10000, 1000000, 0.99, 250, 0., 'adam', 1e-3, 0, 'adam', 1e-4, 10000, True, 0.001, 1, 1.0, False, False, False,
             1, 10)                                                      # keyword-only
    with pytest.raises(NotImplementedError, match="at least one lock-step"):
        make(rollout_steps=0)
    with pytest.raises(NotImplementedError, match="has no rule inside"):
        make(rollout_steps=4, es=ExplorationStrategy())
    # 16384 updates at the most in the one launch behind a chunk: S * n * n_updates_per_sample, S at most an epoch
    make(n_envs=64, rollout_steps=256, epoch_length=64 * 256)
    with pytest.raises(NotImplementedError, match="1 .. 16384"):
        make(n_envs=64, rollout_steps=257, epoch_length=64 * 1000)
    make(n_envs=64, rollout_steps=1000, epoch_length=64 * 256)           # an epoch has 256 lock-steps
    with pytest.raises(NotImplementedError, match="1 .. 16384"):
        make(n_envs=64, rollout_steps=200, n_updates_per_sample=2, epoch_length=64 * 1000)
    with pytest.raises(NotImplementedError, match="replay_pool_size is 100"):
        make(n_envs=8, rollout_steps=13, replay_pool_size=100)
    make(n_envs=8, rollout_steps=12, replay_pool_size=100)


def test_rl_rollout_deterministic_mlp_argument_errors_without_a_device():
    from rllab_amd import _lib
    lib = _lib.lib
    assert lib.rl_rollout_deterministic_mlp(None, None) == -1 and b"rl_rollout_deterministic_mlp" in lib.rl_last_error()
    bounds = (ctypes.c_float * 1)(1.0)

    def args(**kw):
        a = _lib.DetRolloutArgs(kind=_lib.ENV_CARTPOLE, n_envs=70, horizon=5, max_path_length=11, normalize=1,
                                reset_at_start=1, hidden0=32, hidden1=32, hidden_activation=_lib.ACT_RECTIFY,
                                output_activation=_lib.ACT_TANH, explore=_lib.EXPLORE_OU, scale_reward=1.0, ou_theta=0.15,
                                ou_sigma=0.3, low=bounds, high=bounds)
        for name in ("state", "ts", "last_obs", "explore_state", "theta", "sigma_t", "obs", "actions", "means", "rewards",
                     "dones"):
            setattr(a, name, 64)                                         # never dereferenced: every case below is refused
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(n_envs=0), dict(horizon=0), dict(state=None), dict(ts=None), dict(last_obs=None), dict(theta=None),
           dict(obs=None), dict(actions=None), dict(means=None), dict(rewards=None), dict(dones=None),
           dict(hidden0=0), dict(hidden0=65), dict(hidden0=68), dict(hidden0=30), dict(hidden1=0), dict(hidden1=65),
           dict(hidden1=7), dict(hidden_activation=_lib.ACT_IDENTITY), dict(output_activation=_lib.ACT_RECTIFY),
           dict(explore=3), dict(explore=-1), dict(low=None), dict(high=None), dict(explore_state=None),
           dict(explore=_lib.EXPLORE_GAUSSIAN, sigma_t=None), dict(explore=_lib.EXPLORE_GAUSSIAN, low=None),
           dict(kind=99)]
    for kw in bad:
        rc = lib.rl_rollout_deterministic_mlp(ctypes.byref(args(**kw)), None)
        msg = lib.rl_last_error()
        assert rc == -1 and (msg.startswith(b"rl_rollout_deterministic_mlp") or b"env kind 99" in msg), (kw, rc, msg)
    # the soft-constraint steps of the legged envs
    cfg = _lib.env_default_cfg(_lib.ENV_HALF_CHEETAH, flags=_lib.CFG_LIMIT_MUJOCO)
    rc = lib.rl_rollout_deterministic_mlp(ctypes.byref(args(kind=_lib.ENV_HALF_CHEETAH, cfg=ctypes.pointer(cfg))), None)
    assert rc == -2 and b"deterministic rollout" in lib.rl_last_error()
    # more than 32 observations / 8 actions: no env kind has them today, the refusal is compiled per kind


def test_binding_is_documented():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "lib.rl_rollout_deterministic_mlp.argtypes = [vp, vp]" in text
