"""The fused recurrent rollout (rl_rollout_gaussian_gru) and the algorithms on GaussianGRUPolicy.

Parity evidence of the kind the fused rollouts have: the env dynamics replay bit for bit on the host build, the recorded
means sit within 1e-5 of the policy's own float64 forward pass over the recorded planes (``dist_info_planes``, the
definition tests/test_gru_host.py pins against a numpy restatement)."""
import csv
import ctypes
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, MPL = 70, 25, 11          # 70 envs: a partial last wavefront; resets inside the launch
PLANES = ("obs", "actions", "means", "rewards", "dones")


def _policy(kind, hidden, seed=0, scale=0.1, **kw):
    """A GaussianGRUPolicy for env ``kind`` with every parameter -- h0, the biases and log_std too -- moved off its initial
    value."""
    from rllab_amd import _lib
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.spaces import Box
    q = _lib.env_query(kind)
    spec = EnvSpec(Box(-1e6 * np.ones(q["obs_dim"]), 1e6 * np.ones(q["obs_dim"])),
                   Box(-np.ones(q["act_dim"]), np.ones(q["act_dim"])))
    np.random.seed(seed)
    pol = GaussianGRUPolicy(spec, hidden_sizes=(hidden,), **kw)
    theta = pol.get_param_values()
    pol.set_param_values(theta + scale * np.random.RandomState(seed + 1).randn(theta.size))
    return pol


def _noise(q, n, horizon, seed=1):
    rng = np.random.RandomState(seed)
    eps = rng.randn(q["act_dim"], horizon, n).astype(np.float32)
    draws = (rng.randn if q["reset_is_normal"] else rng.rand)(horizon + 1, q["reset_draws"], n).astype(np.float32)
    return eps, draws


def _starts(traj):
    start = torch.ones_like(traj.dones, dtype=torch.bool)
    start[1:] = traj.dones[:-1].bool()
    return start


CASES = [(kind, hidden, True) for kind in (0, 2, 3) for hidden in (32, 20, 64)] + [(2, 32, False)]


@pytest.mark.parametrize("kind,hidden,include_action", CASES)
def test_gru_rollout_parity(kind, hidden, include_action):
    from rllab_amd.envs.hip_env import HipVecEnv
    from oracle.replay import replay_check
    pol = _policy(kind, hidden, state_include_action=include_action)
    v = HipVecEnv(kind, N, MPL, normalize=True, seed=5)
    assert v.takes_rollout_of(pol)
    q = v.q
    eps, draws = _noise(q, N, T)
    traj = v.rollout(pol, T, eps=eps, reset_draws=draws)
    assert v.step_counter == T + 1
    assert replay_check(v, traj, max_envs=N, reset_draws=draws) == N * T
    assert int(traj.dones.sum()) > 0
    # the recorded means against the float64 forward pass over the recorded planes
    flat64 = torch.as_tensor(pol.get_param_values(), dtype=torch.float64, device=traj.device)
    with torch.no_grad():
        d = pol.dist_info_planes(traj.obs.double(), traj.actions.double(), _starts(traj), flat64)
    worst = float((traj.means.double() - d["mean"]).abs().max())
    print("gru means vs float64, kind %d hidden %d include_action %s: max |diff| = %.3e (|mean| max %.3f)" % (
        kind, hidden, include_action, worst, float(d["mean"].abs().max())))
    assert worst <= 1e-5
    # actions == means + eps * exp(log_std), the std in float32 (rounded once from float64), to within one float32 ulp
    ls = pol.get_param_values()[-q["act_dim"]:]
    std32 = np.exp(ls).astype(np.float32).astype(np.float64)[:, None, None]
    act = traj.actions.cpu().numpy()
    want = traj.means.cpu().numpy().astype(np.float64) + eps.astype(np.float64) * std32
    err_ulps = np.abs(act.astype(np.float64) - want) / np.spacing(np.abs(act)).astype(np.float64)
    print("actions vs means + eps * std: max %.3f ulp" % err_ulps.max())
    assert err_ulps.max() <= 1.0
    assert torch.equal(traj.log_std, pol.recorded_log_std())
    # a path carries prev_action = its actions shifted by one step
    if include_action:
        path = __import__("rllab_amd.sampler.trajectories", fromlist=["PathList"]).PathList(traj)[1]
        pa = path["agent_infos"]["prev_action"]
        assert np.all(pa[0] == 0) and np.array_equal(pa[1:], path["actions"][:-1])


def test_gru_rollout_carries_on_without_a_reset():
    """One launch of 25 steps == launches of 10 + 15 on the same envs, the second with reset_at_start=False: every plane and
    the carried buffers bit for bit."""
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 0
    pol = _policy(kind, 32)
    a, b = (HipVecEnv(kind, N, MPL, normalize=True, seed=5) for _ in range(2))
    eps, draws = _noise(a.q, N, T)
    whole = a.rollout(pol, T, eps=eps, reset_draws=draws)
    first = b.rollout(pol, 10, eps=eps[:, :10], reset_draws=draws[:11])
    second = b.rollout(pol, 15, reset_at_start=False, eps=eps[:, 10:], reset_draws=draws[10:])
    assert int(whole.dones[:10].sum()) > 0 and int(whole.dones[10:].sum()) > 0
    assert not bool(whole.dones[9].all())                       # paths run across the cut
    for name in PLANES:
        w = getattr(whole, name)
        got = torch.cat([getattr(first, name), getattr(second, name)], dim=w.dim() - 2)
        assert torch.equal(got, w), name
    for name in ("hidden_state", "prev_action", "state", "ts", "_obs"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert float(a.hidden_state.abs().max()) > 0 and float(a.prev_action.abs().max()) > 0


def test_gru_rollout_philox_path():
    """No injected plane: the same seed and step_counter give the same planes, the next launch differs."""
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 0
    pol = _policy(kind, 32)
    va, vb = (HipVecEnv(kind, N, MPL, normalize=True, seed=9) for _ in range(2))
    a, b = va.rollout(pol, T), vb.rollout(pol, T)
    for name in PLANES:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a2 = va.rollout(pol, T)
    assert va.step_counter == 2 * (T + 1)
    assert not torch.equal(a2.actions, a.actions) and not torch.equal(a2.obs, a.obs)
    assert bool(torch.isfinite(a2.means).all())


def test_gru_rollout_argument_errors_launch_nothing():
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
    theta = torch.zeros(8192, dtype=torch.float32, device=dev)
    cfg = _lib.env_default_cfg(3, flags=_lib.CFG_CONTACT_MUJOCO)

    def call(**kw):
        a = dict(kind=0, n_envs=n, horizon=horizon, max_path_length=5, normalize=1, reset_at_start=1, hidden=H,
                 include_action=1, env_offset=0, scale_reward=1.0, seed=1, step_counter=0, theta=theta.data_ptr())
        a.update({k: t.data_ptr() for k, t in bufs.items()})
        a.update(kw)
        return lib.rl_rollout_gaussian_gru(ctypes.byref(_lib.GruRolloutArgs(**a)), None)

    assert lib.rl_rollout_gaussian_gru(None, None) == -1 and "null" in lib.rl_last_error().decode()
    for kw in (dict(n_envs=0), dict(horizon=0), dict(theta=None), dict(hidden_state=None), dict(prev_action=None),
               dict(last_obs=None), dict(means=None), dict(include_action=2), dict(kind=99)):
        assert call(**kw) == -1, kw
    for hidden in (48, 128, 0):
        assert call(hidden=hidden) == -2 and "hidden = %d" % hidden in lib.rl_last_error().decode()
    assert call(kind=3, cfg=ctypes.pointer(cfg)) == -2 and "soft-constraint" in lib.rl_last_error().decode()
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool(torch.all(t == 7)), name                                   # nothing was launched


# -- the reference's matrix row: the batch algorithms on Cartpole with a GRU policy ---------------------------------------
def _train_logged(algo, tmp_path):
    from rllab_amd.misc import logger
    txt, tab = str(tmp_path / "log.txt"), str(tmp_path / "progress.csv")
    logger.add_text_output(txt)
    logger.add_tabular_output(tab)
    logger.set_quiet(True)
    try:
        algo.train()
    finally:
        logger.remove_text_output(txt)
        logger.remove_tabular_output(tab)
        logger.set_quiet(False)
    with open(tab) as f:
        rows = list(csv.DictReader(f))
    return open(txt).read(), rows


def _algo(name, env, policy, **kw):
    import importlib
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    cls = getattr(importlib.import_module("rllab_amd.algos." + name.lower()), name)
    args = dict(env=env, policy=policy, baseline=ZeroBaseline(env_spec=env.spec), batch_size=1000, max_path_length=100,
                n_itr=1)
    if name in ("TRPO", "TNPG"):
        args["optimizer_args"] = dict(cg_iters=1)
    if name == "PPO":
        args["optimizer_args"] = dict(max_penalty_itr=1, max_opt_itr=1)
    args.update(kw)
    return cls(**args)


@pytest.mark.parametrize("name", ["TRPO", "TNPG", "VPG", "PPO", "ERWR", "TRPO-fd"])
def test_algorithms_on_cartpole_with_a_gru_policy(name, tmp_path):
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    ext.set_seed(1)
    env = CartpoleEnv()
    policy = GaussianGRUPolicy(env_spec=env.spec)
    theta0 = policy.get_param_values()
    if name == "TRPO-fd":
        from rllab_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, FiniteDifferenceHvp
        algo = _algo("TRPO", env, policy, optimizer_args=None,
                     optimizer=ConjugateGradientOptimizer(cg_iters=1, hvp_approach=FiniteDifferenceHvp(base_eps=1e-5)))
    else:
        algo = _algo(name, env, policy)
    text, rows = _train_logged(algo, tmp_path)
    theta = policy.get_param_values()
    assert np.all(np.isfinite(theta)) and theta.shape == theta0.shape
    assert np.array_equal(theta[:32], theta0[:32])                       # h0 is not trainable
    assert "sampling path: fused rollout kernel" in text
    assert "update path: torch autograd -- recurrent policy (no BPTT kernels)" in text
    assert len(rows) == 1 and int(rows[0]["NumTrajs"]) > 0
    assert algo.sampler.last_num_samples >= 1000
    if name in ("TRPO", "TNPG", "PPO", "TRPO-fd"):
        # the update's scan reproduces what the kernel recorded, across launches carried on without a reset
        print(name, "MeanKLBefore", rows[0]["MeanKLBefore"], "MeanKL", rows[0]["MeanKL"])
        assert abs(float(rows[0]["MeanKLBefore"])) < 1e-6


@pytest.mark.parametrize("case,word", [("hidden", "hidden_sizes=(100,)"), ("rectify", "rectify"),
                                       ("normalize_obs", "normalize_obs"), ("reps", "recurrent"),
                                       ("subsample", "subsample_factor")])
def test_gru_refusals(case, word):
    from rllab_amd.algos.reps import REPS
    from rllab_amd.algos.trpo import TRPO
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import logger
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    env = normalize(CartpoleEnv(), normalize_obs=(case == "normalize_obs"))
    kw = dict(hidden=dict(hidden_sizes=(100,)), rectify=dict(hidden_nonlinearity=rectify)).get(case, {})
    policy = GaussianGRUPolicy(env_spec=env.spec, **kw)
    args = dict(env=env, policy=policy, baseline=ZeroBaseline(env_spec=env.spec), batch_size=200, max_path_length=20,
                n_itr=1)
    if case == "subsample":
        args["optimizer_args"] = dict(subsample_factor=0.5)
    algo = (REPS if case == "reps" else TRPO)(**args)
    logger.set_quiet(True)
    try:
        with pytest.raises(NotImplementedError) as e:
            algo.train()
    finally:
        logger.set_quiet(False)
    assert word in str(e.value), str(e.value)


# oracle: tools/exp/trpo_gru_cartpole_cpu.py -- the same configuration on the CPU (host env in float64 sampled path after
# path, float64 autograd update), committed as profiles/curves/trpo_gru_cartpole_cpu.csv
def test_trpo_learns_cartpole_with_a_gru_policy(tmp_path):
    """examples/trpo_gru_cartpole.py's configuration, seed 1.  Every iteration: MeanKL <= 0.0101 and LossAfter <
    LossBefore.  The return: the mean of the last three iterations exceeds the mean of the first three by at least half
    the gain of the CPU yardstick -- half is the margin for the two samplers' different random streams -- and that gain
    is itself positive and at least 20 % of the yardstick's first-three mean."""
    from examples.trpo_gru_cartpole import CONFIG, make_algo
    with open(os.path.join(ROOT, "profiles", "curves", "trpo_gru_cartpole_cpu.csv")) as f:
        cpu = [float(r["AverageReturn"]) for r in csv.DictReader(f)]
    assert len(cpu) == CONFIG["n_itr"]
    cpu_first, cpu_gain = np.mean(cpu[:3]), np.mean(cpu[-3:]) - np.mean(cpu[:3])
    assert cpu_gain > 0 and cpu_gain >= 0.2 * cpu_first, (cpu_first, cpu_gain)
    algo = make_algo(seed=1)
    t0 = time.time()
    text, rows = _train_logged(algo, tmp_path)
    print("wall time %.1f s" % (time.time() - t0))
    assert "sampling path: fused rollout kernel" in text and len(rows) == CONFIG["n_itr"]
    ret = [float(r["AverageReturn"]) for r in rows]
    print("AverageReturn", ret, "CPU", cpu)
    for r in rows:
        print(r["Iteration"], r["LossBefore"], r["LossAfter"], r["MeanKLBefore"], r["MeanKL"])
    for r in rows:
        assert float(r["MeanKL"]) <= 0.0101, r
        assert float(r["LossAfter"]) < float(r["LossBefore"]), r
    assert np.mean(ret[-3:]) - np.mean(ret[:3]) >= 0.5 * cpu_gain, (ret, cpu_gain)
