"""Partially observable tasks on the GPU: DelayedActionEnv's queue inside the fused recurrent rollout
(rl_rollout_gaussian_gru_delayed), OcclusionEnv / Box2DEnv(position_only=True) with a GaussianGRUPolicy laid out on the full
observation, NoisyObservationEnv through ``rl_env_cfg.obs_noise``, the recurrent update kernels on an occluded batch, and the
batch algorithms on examples/trpo_gru_cartpole_po.py's env.

Evidence of the kind tests/test_gpu_gru.py gives: the env dynamics replay bit for bit on the host build when it is fed the
actions that were APPLIED (the recorded ones shifted by the delay inside each path), the executor's per-transition queue
(``HipVecEnv.step``) reproduces the launch bit for bit, the recorded means sit within 1e-5 of the policy's float64 forward
pass, and an occluded executor records the bits of a full-observation executor that runs the scattered parameters.  The
update kernels are held to the rule of tests/test_gpu_gru_bptt.py unchanged (its helpers are used)."""
import csv
import ctypes
import os
import time
import types

import numpy as np
import pytest
import torch

import test_gpu_gru as R
import test_gpu_gru_bptt as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, MPL = R.N, R.T, R.MPL          # 70 envs, 25 steps, paths of at most 11
PLANES = R.PLANES


def _policy(kind, hidden, rows=None, seed=0, scale=0.1, **kw):
    """A GaussianGRUPolicy for env ``kind`` -- on the observation rows ``rows`` when given -- with every parameter moved
    off its initial value."""
    from rllab_amd import _lib
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.spaces import Box
    q = _lib.env_query(kind)
    do = q["obs_dim"] if rows is None else len(rows)
    spec = EnvSpec(Box(-1e6 * np.ones(do), 1e6 * np.ones(do)), Box(-np.ones(q["act_dim"]), np.ones(q["act_dim"])),
                   sensor_rows=None if rows is None else (q["obs_dim"], tuple(rows)))
    np.random.seed(seed)
    pol = GaussianGRUPolicy(spec, hidden_sizes=(hidden,), **kw)
    theta = pol.get_param_values()
    pol.set_param_values(theta + scale * np.random.RandomState(seed + 1).randn(theta.size))
    return pol


def _applied(actions, dones, delay):
    """The actions the envs were stepped with under DelayedActionEnv(delay): inside each path the recorded ones shifted by
    ``delay`` steps, zeros at its start.  numpy [Da, T, n] / [T, n]."""
    out = np.zeros_like(actions)
    steps, n = dones.shape
    for i in range(n):
        p = 0                                     # step index inside the running path
        for t in range(steps):
            if p >= delay:
                out[:, t, i] = actions[:, t - delay, i]
            p = 0 if dones[t, i] else p + 1
    return out


def _check_means_and_actions(pol, traj, eps, what):
    flat64 = torch.as_tensor(pol.get_param_values(), dtype=torch.float64, device=traj.device)
    with torch.no_grad():
        d = pol.dist_info_planes(traj.obs.double(), traj.actions.double(), R._starts(traj), flat64)
    worst = float((traj.means.double() - d["mean"]).abs().max())
    print("%s: means vs float64 max |diff| = %.3e (|mean| max %.3f)" % (what, worst, float(d["mean"].abs().max())))
    assert worst <= 1e-5
    ls = pol.get_param_values()[-pol.action_dim:]
    std32 = np.exp(ls).astype(np.float32).astype(np.float64)[:, None, None]
    act = traj.actions.cpu().numpy()
    want = traj.means.cpu().numpy().astype(np.float64) + eps.astype(np.float64) * std32
    err_ulps = np.abs(act.astype(np.float64) - want) / np.spacing(np.abs(act)).astype(np.float64)
    print("%s: actions vs means + eps * std max %.3f ulp" % (what, err_ulps.max()))
    assert err_ulps.max() <= 1.0


# -- 1. the delayed rollout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delay", [1, 3, 12])
@pytest.mark.parametrize("kind,hidden", [(0, 32), (2, 32), (3, 32), (0, 64), (0, 20)])
def test_delayed_rollout_parity(kind, hidden, delay):
    from rllab_amd.envs.hip_env import HipVecEnv
    from oracle.replay import replay_check
    pol = _policy(kind, hidden)
    v = HipVecEnv(kind, N, MPL, normalize=True, seed=5, action_delay=delay)
    assert v.takes_rollout_of(pol) and not v.graphable
    eps, draws = R._noise(v.q, N, T)
    traj = v.rollout(pol, T, eps=eps, reset_draws=draws)
    assert v.step_counter == T + 1 and int(traj.dones.sum()) > 0
    act, dones = traj.actions.cpu().numpy(), traj.dones.cpu().numpy()
    applied = _applied(act, dones, delay)
    if delay > MPL:
        assert not applied.any()                  # no policy action ever reaches an env
    else:
        assert applied.any() and not np.array_equal(applied, act)
    stand_in = types.SimpleNamespace(T=traj.T, N=traj.N, obs=traj.obs, actions=torch.as_tensor(applied),
                                     rewards=traj.rewards, dones=traj.dones)
    assert replay_check(v, stand_in, max_envs=N, reset_draws=draws) == N * T
    # the policy's side is untouched by the delay: its own actions are what it records and what its GRU is fed
    _check_means_and_actions(pol, traj, eps, "kind %d hidden %d delay %d" % (kind, hidden, delay))
    # what the launch leaves in the queue: the last `delay` actions of the running path, oldest first
    queue = v.action_queue.cpu().numpy()
    longer = np.concatenate([act, np.zeros((act.shape[0], delay, N), np.float32)], axis=1)
    after = _applied(longer, np.concatenate([dones, np.zeros((delay, N), dones.dtype)]), delay)[:, T:]
    assert np.array_equal(queue, after.transpose(1, 0, 2))


# -- 2. the executor's own queue is the definition ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,delay", [(0, 3), (2, 1), (0, 12)])
def test_delayed_rollout_equals_the_per_transition_queue(kind, delay):
    from rllab_amd.envs.hip_env import HipVecEnv
    pol = _policy(kind, 32)
    a, b = (HipVecEnv(kind, N, MPL, normalize=True, seed=5, action_delay=delay) for _ in range(2))
    eps, draws = R._noise(a.q, N, T)
    traj = a.rollout(pol, T, eps=eps, reset_draws=draws)
    obs = b.reset(draws=draws[0])
    for t in range(T):
        assert torch.equal(obs.t(), traj.obs[:, t]), t
        obs, rew, done, _ = b.step(traj.actions[:, t].t(), reset_draws=draws[t + 1])
        assert torch.equal(rew, traj.rewards[t]), t
        assert torch.equal(done, traj.dones[t].bool()), t
    assert torch.equal(obs.t(), a._obs)
    assert torch.equal(b.action_queue, a.action_queue) and tuple(a.action_queue.shape) == (delay, a.q["act_dim"], N)
    for name in ("state", "ts"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # reset(mask) empties the masked columns only
    mask = torch.zeros(N, dtype=torch.bool, device=b.device)
    mask[::2] = True
    before = b.action_queue.clone()
    b.reset(mask=mask)
    assert not bool(b.action_queue[:, :, ::2].any()) and torch.equal(b.action_queue[:, :, 1::2], before[:, :, 1::2])


# -- 3. carrying on ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delay", [3, 4])
def test_delayed_rollout_carries_on_without_a_reset(delay):
    """25 steps == 10 + 15 with reset_at_start=False: 10 % 3 != 0 and 10 % 4 != 0, so the ring is saved mid-turn and comes
    back in logical order."""
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 0
    pol = _policy(kind, 32)
    a, b = (HipVecEnv(kind, N, MPL, normalize=True, seed=5, action_delay=delay) for _ in range(2))
    eps, draws = R._noise(a.q, N, T)
    whole = a.rollout(pol, T, eps=eps, reset_draws=draws)
    first = b.rollout(pol, 10, eps=eps[:, :10], reset_draws=draws[:11])
    cut_queue = b.action_queue.clone()
    second = b.rollout(pol, 15, reset_at_start=False, eps=eps[:, 10:], reset_draws=draws[10:])
    assert int(whole.dones[:10].sum()) > 0 and int(whole.dones[10:].sum()) > 0
    running = ~whole.dones[9].bool()
    assert bool(running.any())                                          # paths run across the cut ...
    assert bool((cut_queue.abs().sum(dim=(0, 1)) > 0)[running].any())   # ... with actions still on their way
    assert not bool(cut_queue[:, :, ~running].any())                    # a finished path leaves an empty queue
    for name in PLANES:
        w = getattr(whole, name)
        got = torch.cat([getattr(first, name), getattr(second, name)], dim=w.dim() - 2)
        assert torch.equal(got, w), name
    for name in ("hidden_state", "prev_action", "state", "ts", "_obs", "action_queue"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert float(a.action_queue.abs().max()) > 0


# -- 4. argument errors -----------------------------------------------------------------------------------------------------------
def test_delayed_rollout_argument_errors_launch_nothing():
    from rllab_amd import _lib
    lib = _lib.lib
    n, horizon, H = 8, 3, 32
    q = _lib.env_query(0)
    dev = torch.device("cuda", 0)
    full = lambda *shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=dev)
    bufs = dict(state=full(q["state_dim"], n), ts=full(n, dtype=torch.int32), last_obs=full(q["obs_dim"], n),
                hidden_state=full(H, n), prev_action=full(q["act_dim"], n), obs=full(q["obs_dim"], horizon, n),
                actions=full(q["act_dim"], horizon, n), means=full(q["act_dim"], horizon, n), rewards=full(horizon, n),
                dones=full(horizon, n, dtype=torch.uint8))
    queue = full(16, q["act_dim"], n)
    theta = torch.zeros(8192, dtype=torch.float32, device=dev)

    def call(delay, qptr, **kw):
        a = dict(kind=0, n_envs=n, horizon=horizon, max_path_length=5, normalize=1, reset_at_start=1, hidden=H,
                 include_action=1, env_offset=0, scale_reward=1.0, seed=1, step_counter=0, theta=theta.data_ptr())
        a.update({k: t.data_ptr() for k, t in bufs.items()})
        a.update(kw)
        return lib.rl_rollout_gaussian_gru_delayed(ctypes.byref(_lib.GruRolloutArgs(**a)), delay, qptr, None)

    assert lib.rl_rollout_gaussian_gru_delayed(None, 3, queue.data_ptr(), None) == -1
    for delay in (0, 17, -1):
        assert call(delay, queue.data_ptr()) == -1 and "action_delay = %d" % delay in lib.rl_last_error().decode()
    assert call(3, None) == -1
    for kw in (dict(n_envs=0), dict(theta=None), dict(prev_action=None), dict(include_action=2), dict(kind=99)):
        assert call(3, queue.data_ptr(), **kw) == -1, kw
    assert call(3, queue.data_ptr(), hidden=48) == -2 and "hidden = 48" in lib.rl_last_error().decode()
    # over-budget LDS: every accepted (kind, hidden, delay) fits -- the largest, Walker2D at 64 units and delay 16, takes
    # 129 KB of the 160 (tests/test_partial_obs_host.py::test_no_accepted_delay_exceeds_the_lds_of_a_cu) -- so that
    # refusal has no case to run here
    torch.cuda.synchronize()
    for name, t in list(bufs.items()) + [("action_queue", queue)]:
        assert bool(torch.all(t == 7)), name                                   # nothing was launched


def test_refusals_under_a_delay():
    from rllab_amd.envs.hip_env import HipVecEnv
    v = HipVecEnv(0, 6, MPL, normalize=True, seed=5, action_delay=2)
    theta = torch.zeros((3, 1217), dtype=torch.float32, device=v.device)
    for call in (lambda: v.rollout_population(theta, 2, 5, 0.99),
                 lambda: v.rollout_population_recurrent(theta, 2, 5, 0.99, 32, True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "DelayedActionEnv" in str(e.value)


# -- 5. occlusion -------------------------------------------------------------------------------------------------------------------
OCCLUDED = [(0, (0, 2), 32), (2, (0, 1, 2, 3, 4), 20), (3, tuple(range(0, 20, 2)), 32)]


@pytest.mark.parametrize("kind,rows,hidden", OCCLUDED)
def test_occluded_rollout_equals_the_scattered_net_on_the_full_observation(kind, rows, hidden):
    from rllab_amd.envs.hip_env import HipVecEnv
    pol = _policy(kind, hidden, rows=rows)
    idx, size = pol.pad_index()
    wide = _policy(kind, pol.kernel_hidden)
    scattered = np.zeros(size)
    scattered[idx] = pol.get_param_values()
    wide.set_param_values(scattered)
    assert torch.equal(pol.rollout_layout(), wide.rollout_layout())
    occ = HipVecEnv(kind, N, MPL, normalize=True, seed=5, position_ids=rows)
    ful = HipVecEnv(kind, N, MPL, normalize=True, seed=5)
    assert occ.takes_rollout_of(pol) and occ.obs_rows == len(rows)
    eps, draws = R._noise(occ.q, N, T)
    a = occ.rollout(pol, T, eps=eps, reset_draws=draws)
    b = ful.rollout(wide, T, eps=eps, reset_draws=draws)
    for name in ("actions", "means", "rewards", "dones"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert tuple(a.obs.shape) == (len(rows), T, N)
    assert torch.equal(a.obs, b.obs.index_select(0, torch.as_tensor(rows, device=b.obs.device)))
    assert int(a.dones.sum()) > 0
    _check_means_and_actions(pol, a, eps, "kind %d rows %r" % (kind, rows))
    # a policy for other rows, or for the full observation, is refused with a sentence
    with pytest.raises(ValueError):
        occ.rollout(wide, T)
    with pytest.raises(ValueError):
        ful.rollout(pol, T)


def test_position_only_and_occlusion_envs_take_the_fused_recurrent_rollout():
    from rllab.envs.occlusion_env import OcclusionEnv
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    for env in (CartpoleEnv(position_only=True), OcclusionEnv(CartpoleEnv(), [0, 2]),
                OcclusionEnv(CartpoleEnv(position_only=True), [1])):
        full, rows = env.spec.sensor_rows
        pol = GaussianGRUPolicy(env_spec=env.spec)
        v = env.vec_env_executor(n_envs=N, max_path_length=MPL, seed=5)
        assert v.position_ids == list(rows) and v.observation_space.flat_dim == len(rows)
        assert v.takes_rollout_of(pol)
        traj = v.rollout(pol, T)
        assert tuple(traj.obs.shape) == (len(rows), T, N) and bool(torch.isfinite(traj.means).all())
        assert tuple(v.reset().shape) == (N, len(rows))


# -- 6. noise -------------------------------------------------------------------------------------------------------------------------
def test_noisy_observation_env_replays_with_the_injected_draws():
    from rllab.envs.noisy_env import NoisyObservationEnv
    from rllab_amd.envs.mujoco.swimmer_env import SwimmerEnv
    from oracle.replay import replay_check
    env = NoisyObservationEnv(SwimmerEnv(), 0.1)
    pol = _policy(2, 32)
    v = env.vec_env_executor(n_envs=N, max_path_length=MPL, seed=5)
    assert v.cfg_overrides["obs_noise"] == 0.1 and abs(float(v.cfg.obs_noise) - 0.1) < 1e-8
    eps, draws = R._noise(v.q, N, T)
    oz = np.random.RandomState(7).randn(T + 1, v.q["obs_dim"], N).astype(np.float32)
    traj = v.rollout(pol, T, eps=eps, reset_draws=draws, obs_noise_z=oz)
    assert replay_check(v, traj, max_envs=N, reset_draws=draws, obs_noise_z=oz) == N * T
    quiet = SwimmerEnv().vec_env_executor(n_envs=N, max_path_length=MPL, seed=5).rollout(pol, T, eps=eps, reset_draws=draws)
    diff = (traj.obs[:, 0] - quiet.obs[:, 0]).cpu().numpy()          # the first observation: the reset state + noise
    assert np.allclose(diff, 0.1 * oz[0], atol=1e-6) and np.abs(diff).max() > 0.1


# -- 7. the update kernels on an occluded batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,rows", [(0, (0, 2)), (2, (0, 1, 2, 3, 4))])
def test_update_kernels_on_an_occluded_batch(kind, rows):
    """Loss, KL, gradient and F v for three directions against float64 autograd of the surr_loss / mean_kl closures on the
    kept rows, by the rule of tests/test_gpu_gru_bptt.py: e_kernel <= 8 max(e_float32_autograd, 2^-20)."""
    pol = _policy(kind, 32, rows=rows, bptt_kernels=True)
    ops = pol.fused_ops()
    assert ops is not None, pol.why_no_kernel_layout()
    assert ops.dims[0] == pol.kernel_obs_dim > pol.obs_dim == len(rows) and ops.index is not None
    inputs = G._planes(pol, N, T)
    assert tuple(inputs[0].shape) == (len(rows), T, N) and ops.accepts(inputs)
    surr, kl = G._closures(pol)
    idx = pol._flat_index(trainable=True)
    l64, g64 = G._grad(pol, surr, inputs, torch.float64)
    l32, g32 = G._grad(pol, surr, inputs, torch.float32)
    with torch.no_grad():
        k64 = kl(pol.flat_params.detach().double(), *G._cast(inputs, torch.float64)).double()
        k32 = kl(pol.flat_params.detach(), *inputs).double()
    l_e, k_e = ops.loss_and_kl(inputs)
    ops.release()
    gk = ops.loss_grad_kernel(inputs, with_loss=True)
    assert (l_e, k_e) == ops.loss_and_kl(inputs)
    t = lambda x: torch.as_tensor([x], dtype=torch.float64)
    G._within("loss", t(l_e), l64.cpu().reshape(1), l32.cpu().reshape(1))
    G._within("KL", t(k_e), k64.cpu().reshape(1), k32.cpu().reshape(1))
    g = ops.gather(gk).double()
    assert g.numel() == ops.n_flat == pol.flat_params.numel() < ops.n_kernel
    G._within("gradient", g[idx], g64[idx], g32[idx])
    # the occluded rows of W_x* (and h0) are places of the kernel layout only: zeros there, never gathered
    pad = torch.ones(ops.n_kernel, dtype=torch.bool, device=gk.device)
    pad[ops.index] = False
    assert int(pad.sum()) == 3 * (pol.kernel_obs_dim - pol.obs_dim) * 32 and bool(torch.all(gk[pad] == 0))
    at_old = G._planes(pol, N, T, at_old=True)
    n, dev = pol.flat_params.numel(), pol.flat_params.device
    rng = np.random.RandomState(11)

    def direction(x):
        v = torch.zeros(n, dtype=torch.float64, device=dev)
        v[idx] = x[idx]
        return v
    dirs = [direction(torch.as_tensor(rng.randn(n), device=dev)), direction(torch.as_tensor(rng.randn(n), device=dev)),
            direction(g64)]
    ops.release()
    got = [ops.fvp(at_old, x) for x in dirs]
    H64 = G._hvp(pol, kl, at_old, torch.float64, dirs)
    H32 = G._hvp(pol, kl, at_old, torch.float32, dirs)
    for name, f, x, h64, h32 in zip("uvg", got, dirs, H64, H32):
        assert f.numel() == n
        G._within("F %s" % name, f[idx], h64[idx], h32[idx])
        assert float(x.dot(f)) > 0
    ops.release()


# -- 8. end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TRPO", "VPG", "PPO", "TRPO-bptt"])
def test_algorithms_on_the_partially_observable_cartpole(name, tmp_path):
    from examples.trpo_gru_cartpole_po import make_env
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    ext.set_seed(1)
    env = make_env()
    assert env.spec.sensor_rows == (4, (0, 2)) and env.spec.observation_space.flat_dim == 2
    policy = GaussianGRUPolicy(env_spec=env.spec, bptt_kernels=(name == "TRPO-bptt"))
    theta0 = policy.get_param_values()
    algo = R._algo(name.split("-")[0], env, policy)
    text, rows = R._train_logged(algo, tmp_path)
    theta = policy.get_param_values()
    assert np.all(np.isfinite(theta)) and theta.shape == theta0.shape and np.abs(theta - theta0).max() > 0
    assert np.array_equal(theta[:32], theta0[:32])                       # h0 is untouched
    assert "sampling path: fused rollout kernel" in text
    assert len(rows) == 1 and int(rows[0]["NumTrajs"]) > 0 and algo.sampler.last_num_samples >= 1000
    v = algo.sampler.vec_env
    assert v.action_delay == 2 and v.position_ids == [0, 2] and v.normalize
    if name == "TRPO-bptt":
        assert "update path: HIP kernels (FusedGRUOps)" in text
        assert "update path: torch autograd for this batch" not in text
        assert float(rows[0]["MeanKLBefore"]) == 0.0
    else:
        assert "update path: torch autograd" in text


def test_a_feed_forward_policy_under_a_delay_is_sampled_per_transition(tmp_path):
    from examples.trpo_gru_cartpole_po import make_env
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(1)
    env = make_env()
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    text, rows = R._train_logged(R._algo("TRPO", env, policy, batch_size=300, max_path_length=20), tmp_path)
    assert "sampling path: per-transition loop (eager)" in text
    assert "DelayedActionEnv: the action queue is built into the recurrent rollout kernel only" in text
    assert len(rows) == 1 and np.all(np.isfinite(policy.get_param_values()))


def test_mlp_policies_stay_on_the_fused_rollout_under_occlusion_and_noise(tmp_path):
    from rllab.envs.noisy_env import NoisyObservationEnv
    from rllab.envs.occlusion_env import OcclusionEnv
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(1)
    env = normalize(NoisyObservationEnv(OcclusionEnv(CartpoleEnv(), [0, 2]), 0.05))
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    algo = R._algo("TRPO", env, policy, batch_size=300, max_path_length=20)
    text, rows = R._train_logged(algo, tmp_path)
    assert "sampling path: fused rollout kernel" in text and len(rows) == 1
    v = algo.sampler.vec_env
    assert v.position_ids == [0, 2] and v.cfg_overrides["obs_noise"] == 0.05


@pytest.mark.parametrize("case", ["normalize_obs", "cem"])
def test_refusals_stay(case):
    from examples.trpo_gru_cartpole_po import make_env
    from rllab.envs.occlusion_env import OcclusionEnv
    from rllab_amd.algos.cem import CEM
    from rllab_amd.algos.trpo import TRPO
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import logger
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    if case == "normalize_obs":
        env = normalize(OcclusionEnv(CartpoleEnv(), [0, 2]), normalize_obs=True)
        policy = GaussianGRUPolicy(env_spec=env.spec)
        algo = TRPO(env=env, policy=policy, baseline=ZeroBaseline(env_spec=env.spec), batch_size=200, max_path_length=20,
                    n_itr=1)
        word = "normalize_obs"
    else:
        env = make_env()
        policy = GaussianGRUPolicy(env_spec=env.spec)
        algo = CEM(env=env, policy=policy, n_itr=1, max_path_length=20, n_samples=8)
        word = "task modifiers"
    logger.set_quiet(True)
    try:
        with pytest.raises(NotImplementedError) as e:
            algo.train()
    finally:
        logger.set_quiet(False)
    assert word in str(e.value), str(e.value)


# -- 9. learning ----------------------------------------------------------------------------------------------------------------------
def test_trpo_learns_the_partially_observable_cartpole(tmp_path):
    """examples/trpo_gru_cartpole_po.py's configuration, seed 1, ten iterations on the recurrent update kernels.  Every
    iteration: MeanKL <= 0.0101 and LossAfter < LossBefore (the conditions of the learning tests of tests/test_gpu_gru.py);
    the mean AverageReturn of the last three iterations exceeds that of the first three.  The curve goes to
    profiles/curves/trpo_gru_cartpole_po.csv, for the record."""
    from examples.trpo_gru_cartpole_po import CONFIG, make_algo
    algo = make_algo(seed=1, bptt_kernels=True)
    t0 = time.time()
    text, rows = R._train_logged(algo, tmp_path)
    print("wall time %.1f s" % (time.time() - t0))
    assert "sampling path: fused rollout kernel" in text and "update path: HIP kernels (FusedGRUOps)" in text
    assert len(rows) == CONFIG["n_itr"] == 10
    ret = [float(r["AverageReturn"]) for r in rows]
    print("AverageReturn", ret)
    for r in rows:
        print(r["Iteration"], r["LossBefore"], r["LossAfter"], r["MeanKLBefore"], r["MeanKL"])
    with open(os.path.join(ROOT, "profiles", "curves", "trpo_gru_cartpole_po.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Iteration", "AverageReturn", "LossBefore", "LossAfter", "MeanKL"])
        for r in rows:
            w.writerow([r["Iteration"], r["AverageReturn"], r["LossBefore"], r["LossAfter"], r["MeanKL"]])
    for r in rows:
        assert float(r["MeanKL"]) <= 0.0101, r
        assert float(r["LossAfter"]) < float(r["LossBefore"]), r
    assert np.mean(ret[-3:]) > np.mean(ret[:3]), ret
