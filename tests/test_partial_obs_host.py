"""The partially observable task modifiers on the host (no GPU): OcclusionEnv, NoisyObservationEnv, DelayedActionEnv
(rllab/envs/occlusion_env.py, rllab/envs/noisy_env.py), ``EnvSpec.sensor_rows``, and the GRU kernel layout of a policy
built on kept observation rows."""
import os
import pickle

import numpy as np
import pytest
import torch


def _cartpole(**kw):
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    return CartpoleEnv(**kw)


# -- OcclusionEnv -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sensor_idx,rows", [([0, 2], (0, 2)), ([2, 0], (0, 2)), ([True, False, True, False], (0, 2)),
                                             ([1, 0, 1, 0], (0, 2)), (np.array([3]), (3,)), ([0, 1, 2, 3], (0, 1, 2, 3))])
def test_occlusion_mask_forms(sensor_idx, rows):
    from rllab.envs.occlusion_env import OcclusionEnv
    env = OcclusionEnv(_cartpole(), sensor_idx)
    assert env.sensor_rows == (4, rows)
    assert env.observation_space.flat_dim == len(rows)
    assert np.array_equal(env.observation_space.bounds[1], 1e6 * np.ones(len(rows)))
    assert np.array_equal(env.observation_space.bounds[0], -1e6 * np.ones(len(rows)))
    assert np.array_equal(env.occlude(np.arange(4.0)), np.asarray(rows, dtype=np.float64))
    assert env.spec.sensor_rows == (4, rows) and env.spec.observation_space.flat_dim == len(rows)
    assert env.vectorized and env.action_space.flat_dim == 1
    assert env.log_diagnostics([dict(observations=np.zeros((3, len(rows))))]) is None


@pytest.mark.parametrize("sensor_idx", [[0, 1, 2, 3, 0], [0, 2, 2], [True, False, True]])
def test_occlusion_errors(sensor_idx):
    """The reference's three: longer than the observation, a repeated index, a boolean mask that is too short."""
    from rllab.envs.occlusion_env import OcclusionEnv
    with pytest.raises(ValueError):
        OcclusionEnv(_cartpole(), sensor_idx)


def test_occlusion_composes_with_position_only():
    from rllab.envs.noisy_env import DelayedActionEnv, NoisyObservationEnv
    from rllab.envs.occlusion_env import OcclusionEnv
    inner = _cartpole(position_only=True)
    shown = inner.spec.sensor_rows
    assert shown is not None and shown[0] == 4 and len(shown[1]) == inner.observation_space.flat_dim
    assert _cartpole().spec.sensor_rows is None
    for k in range(len(shown[1])):
        env = OcclusionEnv(inner, [k])
        assert env.sensor_rows == (4, (shown[1][k],))
    # the rows travel through the other two modifiers and normalize
    from rllab_amd.envs.normalized_env import normalize
    env = normalize(DelayedActionEnv(NoisyObservationEnv(OcclusionEnv(_cartpole(), [1, 3]), 0.2), action_delay=4))
    assert env.spec.sensor_rows == (4, (1, 3)) and env.spec.observation_space.flat_dim == 2
    assert normalize(NoisyObservationEnv(_cartpole())).spec.sensor_rows is None


# -- the three wrappers ---------------------------------------------------------------------------------------------------------
def test_pickle_round_trips():
    from rllab.envs.noisy_env import DelayedActionEnv, NoisyObservationEnv
    from rllab.envs.occlusion_env import OcclusionEnv
    o = pickle.loads(pickle.dumps(OcclusionEnv(_cartpole(), [0, 2])))
    assert o.sensor_rows == (4, (0, 2)) and o.observation_space.flat_dim == 2
    n = pickle.loads(pickle.dumps(NoisyObservationEnv(_cartpole(), obs_noise=0.25)))
    assert n.obs_noise == 0.25 and n.observation_space.flat_dim == 4 and NoisyObservationEnv(_cartpole()).obs_noise == 0.1
    d = pickle.loads(pickle.dumps(DelayedActionEnv(_cartpole(), action_delay=5)))
    assert d.action_delay == 5 and DelayedActionEnv(_cartpole()).action_delay == 3
    all3 = pickle.loads(pickle.dumps(DelayedActionEnv(NoisyObservationEnv(OcclusionEnv(_cartpole(), [0, 2]), 0.3), 2)))
    assert (all3.action_delay, all3.wrapped_env.obs_noise, all3.wrapped_env.wrapped_env.sensor_rows) == (2, 0.3, (4, (0, 2)))
    spec = pickle.loads(pickle.dumps(all3.spec))
    assert spec.sensor_rows == (4, (0, 2)) and spec.observation_space.flat_dim == 2


def test_wrapper_refusals():
    from rllab.envs.noisy_env import DelayedActionEnv, NoisyObservationEnv
    from rllab.envs.occlusion_env import OcclusionEnv
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            DelayedActionEnv(_cartpole(), action_delay=bad)
    with pytest.raises(ValueError) as e:
        NoisyObservationEnv(_cartpole(obs_noise=0.05), 0.1)
    assert "two independent draws" in str(e.value)
    with pytest.raises(ValueError) as e:
        DelayedActionEnv(NoisyObservationEnv(DelayedActionEnv(_cartpole())))
    assert "at most one of each kind" in str(e.value)
    for make in (lambda g: OcclusionEnv(g, [0]), NoisyObservationEnv, DelayedActionEnv):
        with pytest.raises(NotImplementedError) as e:
            make(GridWorldEnv())
        assert "GridWorldEnv" in str(e.value)


class _Recorder(object):
    """Stands where the HIP env's single-env face is: deterministic observations, the applied actions on record."""

    def __init__(self):
        self.applied, self.t = [], 0

    def reset(self):
        self.t = 0
        return np.arange(4.0)

    def step(self, action):
        from rllab_amd.envs.base import Step
        self.applied.append(np.array(action, dtype=np.float64))
        self.t += 1
        return Step(np.arange(4.0) + self.t, 1.0, False)

    def get_current_obs(self):
        return np.arange(4.0) + self.t


def _over_recorder(env):
    from rllab_amd.envs.hip_env import HipEnv
    rec = _Recorder()
    base = env
    while not isinstance(base._wrapped_env, HipEnv):
        base = base._wrapped_env
    rec.action_space = base._wrapped_env.action_space
    base._wrapped_env = rec
    return rec


def test_single_env_face_in_numpy():
    from rllab.envs.noisy_env import DelayedActionEnv, NoisyObservationEnv
    from rllab.envs.occlusion_env import OcclusionEnv
    env = DelayedActionEnv(NoisyObservationEnv(OcclusionEnv(_cartpole(), [1, 3]), 0.5), action_delay=2)
    rec = _over_recorder(env)
    np.random.seed(3)
    z = np.random.RandomState(3).normal(size=(4, 2))
    first = env.reset()
    assert np.array_equal(first, np.array([1.0, 3.0]) + 0.5 * z[0])
    for t in range(3):
        step = env.step(np.array([t + 1.0]))
        assert np.array_equal(step.observation, np.array([1.0, 3.0]) + (t + 1) + 0.5 * z[t + 1])
        assert step.reward == 1.0 and step.done is False
    # zeros for the first `action_delay` steps, then the actions in the order they were given
    assert [float(a[0]) for a in rec.applied] == [0.0, 0.0, 1.0]
    env.reset()
    env.step(np.array([9.0]))
    assert float(rec.applied[-1][0]) == 0.0                      # reset emptied the queue
    with pytest.raises(RuntimeError):
        DelayedActionEnv(_cartpole(), 1).step(np.zeros(1))


# -- the kernel layout of a policy on kept rows ---------------------------------------------------------------------------------
def _spec(do, da, sensor_rows=None):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Box
    return EnvSpec(Box(-np.ones(do), np.ones(do)), Box(-np.ones(da), np.ones(da)), sensor_rows=sensor_rows)


def _policy(spec, hidden, seed=0, **kw):
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    np.random.seed(seed)
    pol = GaussianGRUPolicy(spec, hidden_sizes=(hidden,), **kw)
    theta = pol.get_param_values()
    pol.set_param_values(theta + 0.3 * np.random.RandomState(seed + 1).randn(theta.size))
    return pol


CASES = [(4, 1, (0, 2), 32, True), (13, 2, (0, 1, 2, 3, 4), 20, True), (20, 6, tuple(range(0, 20, 2)), 64, False),
         (4, 1, (3, 1), 20, True)]


def _np_pad_index(full, ids, da, H, Hp, include_action):
    """The kernel vector written out: h0 [Hp]; per gate W_x [full (+ da)][Hp], W_h [Hp][Hp], b [Hp]; W_out [Hp][da];
    b_out [da]; log_std [da].  Returns (position of every flat parameter, in flat order; size)."""
    k = len(ids)
    di_flat, di_kernel = k + (da if include_action else 0), full + (da if include_action else 0)
    pos, off = [], 0
    pos += [off + j for j in range(H)]
    off += Hp
    for _ in range(3):
        for r in range(di_flat):
            row = ids[r] if r < k else full + (r - k)
            pos += [off + row * Hp + j for j in range(H)]
        off += di_kernel * Hp
        for r in range(H):
            pos += [off + r * Hp + j for j in range(H)]
        off += Hp * Hp
        pos += [off + j for j in range(H)]
        off += Hp
    for r in range(H):
        pos += [off + r * da + j for j in range(da)]
    off += Hp * da
    pos += [off + j for j in range(da)]
    off += da
    pos += [off + j for j in range(da)]
    off += da
    return np.asarray(pos), off


@pytest.mark.parametrize("full,da,ids,hidden,include_action", CASES)
def test_pad_index_with_sensor_rows(full, da, ids, hidden, include_action):
    pol = _policy(_spec(len(ids), da, (full, ids)), hidden, state_include_action=include_action)
    assert pol.sensor_rows == (full, tuple(ids)) and pol.kernel_obs_dim == full and pol.obs_dim == len(ids)
    assert not pol.kernel_layout_is_flat
    idx, size = pol.pad_index()
    want, want_size = _np_pad_index(full, ids, da, hidden, pol.kernel_hidden, include_action)
    assert size == want_size and np.array_equal(idx, want)
    assert len(np.unique(idx)) == idx.size == pol.get_param_values().size
    # pack_rows: the same scatter on rows, zeros everywhere else
    xs = torch.as_tensor(np.random.RandomState(2).randn(3, idx.size), dtype=torch.float32, device=pol.flat_params.device)
    rows = pol.pack_rows(xs).cpu().numpy()
    assert rows.shape == (3, size) and np.array_equal(rows[:, idx], xs.cpu().numpy())
    assert np.count_nonzero(rows) == np.count_nonzero(xs.cpu().numpy())
    # without sensor rows nothing changes
    plain = _policy(_spec(full, da), hidden, state_include_action=include_action)
    assert plain.sensor_rows is None and plain.kernel_obs_dim == full
    assert plain.kernel_layout_is_flat == (hidden == plain.kernel_hidden)


def test_sensor_rows_are_checked():
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    for rows in ((4, (0, 1, 2)), (4, (0, 0)), (4, (0, 4))):
        with pytest.raises(ValueError):
            GaussianGRUPolicy(_spec(2, 1, rows))


@pytest.mark.parametrize("full,da,ids,hidden,include_action", CASES)
def test_forward_on_kept_rows_equals_scattered_net_on_full_observation(full, da, ids, hidden, include_action):
    """float64 ``dist_info_planes`` of the policy on its kept rows == the same parameters scattered into the kernel
    layout, read as a policy on the FULL observation at ``kernel_hidden`` units, on full observations whose occluded
    rows hold arbitrary finite values."""
    pol = _policy(_spec(len(ids), da, (full, ids)), hidden, state_include_action=include_action)
    idx, size = pol.pad_index()
    wide = _policy(_spec(full, da), pol.kernel_hidden, state_include_action=include_action)
    assert wide.kernel_layout_is_flat and wide.get_param_values().size == size
    scattered = np.zeros(size)
    scattered[idx] = pol.get_param_values()
    rng = np.random.RandomState(5)
    T, N = 9, 6
    obs_full = torch.as_tensor(rng.randn(full, T, N) * 100.0)
    actions = torch.as_tensor(rng.randn(da, T, N))
    start = torch.as_tensor(rng.rand(T, N) < 0.2)
    start[0] = True
    kept = torch.as_tensor(list(ids), dtype=torch.long)
    with torch.no_grad():
        a = pol.dist_info_planes(obs_full.index_select(0, kept), actions, start,
                                 torch.as_tensor(pol.get_param_values(), dtype=torch.float64))
        b = wide.dist_info_planes(obs_full, actions, start, torch.as_tensor(scattered, dtype=torch.float64))
    assert a["mean"].shape == b["mean"].shape == (da, T, N)
    assert float((a["mean"] - b["mean"]).abs().max()) <= 1e-12 * max(1.0, float(a["mean"].abs().max()))
    assert torch.equal(a["log_std"], b["log_std"])


# -- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_delayed_entry_point_is_exported():
    from rllab_amd import _lib
    assert "rl_rollout_gaussian_gru_delayed" in _lib.SYMBOLS
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rllab_amd.h")) as f:
        assert "int rl_rollout_gaussian_gru_delayed(const rl_gru_rollout_args* args, int32_t action_delay, " \
               "float* action_queue, void* stream);" in f.read()
    assert _lib.lib.rl_rollout_gaussian_gru_delayed(None, 3, None, None) == -1
    assert "null" in _lib.lib.rl_last_error().decode()
    assert _lib.lib.rl_abi_version() == 14
    assert _lib.lib.rl_rollout_gaussian_gru_delayed.argtypes[0]._type_ is _lib.GruRolloutArgs


def test_a_queued_zero_reaches_every_env_as_raw_zero():
    """normalize's action map lb + (a + 1) 0.5 (ub - lb) is applied to whatever reaches the env, a queued zero included,
    where the reference (normalize OUTSIDE DelayedActionEnv) applies the raw zero.  The bounds of all eight kinds are
    symmetric, so the map takes 0 to +0 exactly in float32, with or without a fused multiply-add."""
    from rllab_amd import _lib
    f = np.float32
    for kind in range(8):
        lb, ub = (np.asarray(b, dtype=np.float32) for b in _lib.env_action_bounds(kind))
        assert np.array_equal(lb, -ub) and np.all(ub > 0), kind
        half = (f(0.0) + f(1.0)) * f(0.5)
        plain = lb + half * (ub - lb)
        fused = (lb.astype(np.float64) + np.float64(half) * (ub - lb).astype(np.float64)).astype(np.float32)   # one rounding
        for out in (plain, fused, np.clip(plain, lb, ub)):
            assert np.all(out == 0) and not np.any(np.signbit(out)), (kind, out)


def test_no_accepted_delay_exceeds_the_lds_of_a_cu():
    """The LDS of rl_rollout_gaussian_gru_delayed -- parameters, two [H][64] tiles, the [delay * Da][64] ring -- for every
    env kind at 64 units and the largest accepted delay: all below 160 KB, so the entry point's over-budget refusal
    cannot be reached through an accepted (kind, hidden, delay) today; the check stays for wider envs."""
    from rllab_amd import _lib
    worst = 0
    for kind in range(8):
        q = _lib.env_query(kind)
        H, do, da = 64, q["obs_dim"], q["act_dim"]
        floats = H + 3 * ((do + da) * H + H * H + H) + H * da + da + da + 16 * da * 64
        worst = max(worst, 4 * (4 * -(-floats // 4) + 2 * H * 64))
    assert worst <= 160 * 1024, worst
