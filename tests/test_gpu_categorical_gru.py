"""The fused recurrent GridWorld rollout (rl_rollout_gridworld_gru) and the algorithms on CategoricalGRUPolicy -- the
reference's matrix row GridWorldEnv + CategoricalGRUPolicy (tests/test_algos.py:76-94 of rllab).

Parity evidence of the kind the other fused rollouts have: the recorded planes replay on the Python GridWorldEnv (integers:
equality), the recorded probabilities sit within 1e-5 of the policy's own float64 forward pass over the recorded planes
(``dist_info_planes``, the definition tests/test_categorical_gru_host.py pins against a numpy restatement) -- a plain
float32 evaluation of that scan on the CPU at these shapes and this parameter scale sits at 8e-8, so the bar leaves the
kernel's fast exp2 / rcp two orders of magnitude -- and the recorded action is the cumulative rule in float32 on the
recorded probabilities (equality)."""
import csv
import ctypes
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, MPL = 70, 40, 11          # 70 envs: one full wavefront plus 6 lanes; paths end by hole / goal and by the horizon
PLANES = ("obs", "actions", "means", "rewards", "dones")
CARRIED = ("state", "ts", "hidden_state", "prev_action")


def _policy(desc, hidden=32, seed=0, **kw):
    """(GridWorldEnv, CategoricalGRUPolicy) with every parameter -- h0 and the biases too -- moved off its initial value."""
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    env = GridWorldEnv(desc)
    np.random.seed(seed)
    pol = CategoricalGRUPolicy(env.spec, hidden_dim=hidden, **kw)
    theta = pol.get_param_values()
    pol.set_param_values(theta + 0.1 * np.random.RandomState(seed + 1).randn(theta.size))
    return env, pol


def _uniforms(steps, n, seed=7):
    return np.minimum(np.random.RandomState(seed).rand(steps, n).astype(np.float32), np.float32(1 - 2.0 ** -24))


def _starts(traj):
    start = torch.ones_like(traj.dones, dtype=torch.bool)
    start[1:] = traj.dones[:-1].bool()
    return start


def _replay(env, traj_chunks, n, max_path_length):
    """Every env's recorded actions through the Python GridWorldEnv with the executor's reset rule; asserts observations,
    rewards and dones of all chunks (consecutive launches of the same envs) and returns the final (state, ts) lists."""
    obs = np.concatenate([c.obs.cpu().numpy() for c in traj_chunks], axis=1)
    act = np.concatenate([c.actions.cpu().numpy() for c in traj_chunks], axis=1)
    rew = np.concatenate([c.rewards.cpu().numpy() for c in traj_chunks], axis=0)
    done = np.concatenate([c.dones.cpu().numpy() for c in traj_chunks], axis=0)
    assert set(np.unique(obs)) <= {0.0, 1.0} and np.all(obs.sum(axis=0) == 1) and np.all(act.sum(axis=0) == 1)
    steps = rew.shape[0]
    states, tss = [], []
    for i in range(n):
        s, ts = env.reset(), 0
        for t in range(steps):
            assert int(np.argmax(obs[:, t, i])) == s, (i, t)
            o, r, d, _ = env.step(int(np.argmax(act[:, t, i])))
            ts += 1
            d = bool(d) or ts >= max_path_length
            assert float(rew[t, i]) == float(r) and bool(done[t, i]) == d, (i, t)
            if d:
                o, ts = env.reset(), 0
            s = o
        states.append(s)
        tss.append(ts)
    return states, tss


# -- parity -----------------------------------------------------------------------------------------------------------------
CASES = [("4x4", 32, True), ("4x4_safe", 32, True), ("chain", 32, True), ("4x4", 20, True), ("4x4", 64, True),
         ("8x8", 64, True), ("4x4", 32, False)]


@pytest.mark.parametrize("desc,hidden,include_action", CASES)
def test_rollout_parity(desc, hidden, include_action):
    from rllab_amd.sampler.trajectories import PathList
    env, pol = _policy(desc, hidden, state_include_action=include_action)
    ve = env.vec_env_executor(N, MPL, seed=3)
    assert ve.takes_rollout_of(pol) and pol.why_no_rollout_kernel() is None
    S = env.observation_space.n
    u = _uniforms(T, N)
    traj = ve.rollout(pol, T, reset_at_start=True, u=u)
    assert traj.categorical and traj.log_std is None and traj.prev_action_info == include_action
    assert (traj.T, traj.N, traj.obs_dim, traj.act_dim) == (T, N, S, 4) and ve.step_counter == T
    assert tuple(ve.hidden_state.shape) == (pol.kernel_hidden, N) and ve.prev_action.dtype == torch.int32
    # the env: observations, rewards, dones and the carried state / step count replay on the Python env
    states, tss = _replay(env, [traj], N, MPL)
    assert ve.state.cpu().tolist() == states and ve.ts.cpu().tolist() == tss
    # the recorded probabilities against the float64 forward pass over the recorded planes
    prob = traj.means
    flat64 = torch.as_tensor(pol.get_param_values(), dtype=torch.float64, device=traj.device)
    with torch.no_grad():
        want = pol.dist_info_planes(traj.obs.double(), traj.actions.double(), _starts(traj), flat64)["prob"]
    worst = float((prob.double() - want).abs().max())
    sums = float((prob.double().sum(dim=0) - 1).abs().max())
    print("gru prob vs float64, %s hidden %d include_action %s: max |diff| = %.3e, max |row sum - 1| = %.3e" % (
        desc, hidden, include_action, worst, sums))
    assert worst <= 1e-5
    assert sums <= 1e-6
    # the recorded action: the cumulative rule in float32 on the recorded probabilities
    p = prob.cpu().numpy()
    assert p.dtype == np.float32 and np.cumsum(p, axis=0).dtype == np.float32
    act_idx = np.minimum((np.cumsum(p, axis=0) < u[None]).sum(axis=0), 3)
    assert np.array_equal(traj.actions.cpu().numpy().argmax(axis=0), act_idx)
    assert len(np.unique(act_idx)) == 4 and int(traj.dones.sum()) > N         # every action taken, every env ended paths
    # the carried previous action: the last action's index, -1 where the last step ended a path
    last_done = traj.dones[-1].bool().cpu().numpy()
    assert np.array_equal(ve.prev_action.cpu().numpy(), np.where(last_done, -1, act_idx[-1]))
    # a path carries prev_action = its one-hot actions shifted by one step, zeros first
    paths = PathList(traj)
    path = paths[1]
    assert set(path["agent_infos"]) == ({"prob", "prev_action"} if include_action else {"prob"})
    if include_action:
        pa = path["agent_infos"]["prev_action"]
        assert pa.shape == path["actions"].shape and np.all(pa[0] == 0) and np.array_equal(pa[1:], path["actions"][:-1])


def test_rollout_carries_on_without_a_reset():
    """One launch of 25 steps == launches of 10 + 15 on the same envs, the second with reset_at_start=False: every plane and
    the carried buffers bit for bit."""
    env, pol = _policy("4x4", 32)
    a, b = (env.vec_env_executor(N, MPL, seed=5) for _ in range(2))
    u = _uniforms(25, N, seed=2)
    whole = a.rollout(pol, 25, u=u)
    first = b.rollout(pol, 10, u=u[:10])
    second = b.rollout(pol, 15, reset_at_start=False, u=u[10:])
    assert int(whole.dones[:10].sum()) > 0 and int(whole.dones[10:].sum()) > 0
    assert not bool(whole.dones[9].all())                       # paths run across the cut
    for name in PLANES:
        w = getattr(whole, name)
        got = torch.cat([getattr(first, name), getattr(second, name)], dim=w.dim() - 2)
        assert torch.equal(got, w), name
    for name in CARRIED:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert float(a.hidden_state.abs().max()) > 0 and int(a.prev_action.max()) > 0 and a.step_counter == b.step_counter == 25
    _replay(env, [first, second], N, MPL)
    # a fresh executor has no hidden state to carry on from
    with pytest.raises(ValueError):
        env.vec_env_executor(N, MPL, seed=5).rollout(pol, 5, reset_at_start=False)


def test_philox_rollout_is_a_function_of_seed_and_counter():
    env, pol = _policy("4x4", 32)
    a, b = (env.vec_env_executor(200, 20, seed=5) for _ in range(2))
    ta, tb = a.rollout(pol, 25), b.rollout(pol, 25)
    for name in PLANES:
        assert torch.equal(getattr(ta, name), getattr(tb, name)), name
    ta2 = a.rollout(pol, 25)                                     # the next launch: the next 25 counters
    assert a.step_counter == 50
    assert not torch.equal(ta2.actions, ta.actions) and bool(torch.isfinite(ta2.means).all())
    # env_offset shifts the streams: envs 100 .. 199 of one executor are envs 0 .. 99 of one that starts at 100
    e = env.vec_env_executor(100, 20, seed=5, env_offset=100).rollout(pol, 25)
    for name in PLANES:
        assert torch.equal(getattr(e, name), getattr(ta, name)[..., 100:]), name


def test_philox_first_step_frequencies():
    """A five-sigma condition on a correct sampler at one fixed seed: |freq - p| <= 5 sqrt(p (1 - p) / n).  At t = 0 every
    env has h0 and no previous action, so one probability vector applies."""
    n = 65536
    env, pol = _policy("4x4", 32, seed=4)
    ve = env.vec_env_executor(n, 10, seed=12345)
    traj = ve.rollout(pol, 1)
    first = traj.means[:, 0, :]
    assert bool((first == first[:, :1]).all())
    p = first[:, 0].double().cpu().numpy()
    freq = traj.actions[:, 0, :].double().mean(dim=1).cpu().numpy()
    for k in range(4):
        assert abs(freq[k] - p[k]) <= 5 * np.sqrt(p[k] * (1 - p[k]) / n), (k, freq[k], p[k])


def test_argument_errors_launch_nothing():
    from rllab_amd import _lib
    lib = _lib.lib
    n, horizon, H, S = 8, 3, 32, 16
    dev = torch.device("cuda", 0)
    full = lambda *shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=dev)
    bufs = dict(state=full(n, dtype=torch.int32), ts=full(n, dtype=torch.int32), hidden_state=full(64, n),
                prev_action=full(n, dtype=torch.int32), obs=full(S, horizon, n), actions=full(4, horizon, n),
                prob_out=full(4, horizon, n), rewards=full(horizon, n), dones=full(horizon, n, dtype=torch.uint8))
    theta = torch.zeros(65536, dtype=torch.float32, device=dev)
    cell = torch.zeros(S, dtype=torch.int8, device=dev)

    def call(**kw):
        a = dict(n_envs=n, horizon=horizon, max_path_length=5, reset_at_start=1, n_row=4, n_col=4, n_act=4, start_state=0,
                 env_offset=0, hidden=H, include_action=1, seed=1, step_counter=0, cell=cell.data_ptr(),
                 theta=theta.data_ptr())
        a.update({k: t.data_ptr() for k, t in bufs.items()})
        a.update(kw)
        return lib.rl_rollout_gridworld_gru(ctypes.byref(_lib.GridWorldGruArgs(**a)), None)

    assert lib.rl_rollout_gridworld_gru(None, None) == -1 and "null" in lib.rl_last_error().decode()
    for kw in (dict(n_envs=0), dict(horizon=0), dict(theta=None), dict(hidden_state=None), dict(prev_action=None),
               dict(prob_out=None), dict(include_action=2), dict(n_act=5), dict(start_state=16), dict(start_state=-1)):
        assert call(**kw) == -1, kw
    for hidden in (48, 128, 0):
        assert call(hidden=hidden) == -2 and "hidden = %d" % hidden in lib.rl_last_error().decode()
    # a map too large for the LDS of a CU: the message names the byte count
    for rows, cols, hidden, include_action in ((20, 20, 32, 1), (8, 16, 64, 0)):
        assert call(n_row=rows, n_col=cols, hidden=hidden, include_action=include_action) == -2
        di = rows * cols + 4 * include_action
        need = 4 * (hidden + 3 * (di * hidden + hidden * hidden + hidden) + 4 * hidden + 4 + 2 * hidden * 64)
        msg = lib.rl_last_error().decode()
        assert need > 160 * 1024 and "%d bytes of LDS" % need in msg, msg
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool(torch.all(t == 7)), name                                   # nothing was launched


# -- the reference's matrix row: the batch algorithms on GridWorld with a GRU policy ----------------------------------------
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


@pytest.mark.parametrize("name", ["TRPO", "TNPG", "VPG", "PPO", "TRPO-fd"])
def test_algorithms_on_gridworld_with_a_gru_policy(name, tmp_path):
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    ext.set_seed(1)
    env = GridWorldEnv()
    policy = CategoricalGRUPolicy(env_spec=env.spec)
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
    ent = float(rows[0]["Entropy"])
    assert 0 < ent <= np.log(4)
    assert "AveragePolicyStd" not in rows[0]                               # nothing Gaussian is logged
    if name in ("TRPO", "TNPG", "PPO", "TRPO-fd"):
        # the update's scan reproduces what the kernel recorded, across launches carried on without a reset
        print(name, "MeanKLBefore", rows[0]["MeanKLBefore"], "MeanKL", rows[0]["MeanKL"])
        assert abs(float(rows[0]["MeanKLBefore"])) < 1e-6


@pytest.mark.parametrize("name", ["ERWR", "REPS", "CEM"])
def test_algorithms_without_a_recurrent_categorical_path_say_so(name):
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import logger
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    env = GridWorldEnv()
    policy = CategoricalGRUPolicy(env_spec=env.spec)
    if name == "CEM":
        from rllab_amd.algos.cem import CEM
        algo = CEM(env=env, policy=policy, n_itr=1, max_path_length=100)
    else:
        algo = _algo(name, env, policy)
    logger.set_quiet(True)
    try:
        with pytest.raises(NotImplementedError):
            algo.train()
    finally:
        logger.set_quiet(False)


@pytest.mark.parametrize("case,word", [("hidden", "hidden_dim=100"), ("rectify", "rectify")])
def test_policies_the_kernel_does_not_run_are_refused_at_start_worker(case, word):
    from rllab_amd.algos.trpo import TRPO
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import logger
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    env = GridWorldEnv()
    kw = dict(hidden=dict(hidden_dim=100), rectify=dict(hidden_nonlinearity=rectify))[case]
    policy = CategoricalGRUPolicy(env_spec=env.spec, **kw)
    assert word in policy.why_no_rollout_kernel()
    algo = TRPO(env=env, policy=policy, baseline=ZeroBaseline(env_spec=env.spec), batch_size=200, max_path_length=20, n_itr=1)
    logger.set_quiet(True)
    try:
        with pytest.raises(NotImplementedError) as e:
            algo.start_worker()
    finally:
        logger.set_quiet(False)
    assert word in str(e.value) and policy.why_no_rollout_kernel() in str(e.value), str(e.value)


# oracle: tools/exp/trpo_gridworld_gru_cpu.py -- the same configuration on the CPU (the Python env sampled path after path
# with the host get_action, float64 autograd update), committed as profiles/curves/trpo_gridworld_gru_cpu.csv
def test_trpo_learns_gridworld_with_a_gru_policy(tmp_path):
    """examples/trpo_gridworld_gru.py's configuration, seed 1.  Every iteration: MeanKL <= 0.0101, LossAfter < LossBefore
    and |MeanKLBefore| < 1e-6.  The return (a success rate in [0, 1]): the mean of the last three iterations exceeds the
    mean of the first three by at least half the gain of the CPU yardstick -- half is the margin for the two samplers'
    different random streams -- and that gain is itself at least 0.2."""
    from examples.trpo_gridworld_gru import CONFIG, make_algo
    with open(os.path.join(ROOT, "profiles", "curves", "trpo_gridworld_gru_cpu.csv")) as f:
        cpu = [float(r["AverageReturn"]) for r in csv.DictReader(f)]
    assert len(cpu) == CONFIG["n_itr"] <= 15 and CONFIG["batch_size"] <= 4000
    cpu_gain = np.mean(cpu[-3:]) - np.mean(cpu[:3])
    assert cpu_gain >= 0.2, cpu
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
        assert abs(float(r["MeanKLBefore"])) < 1e-6, r
    assert np.mean(ret[-3:]) - np.mean(ret[:3]) >= 0.5 * cpu_gain, (ret, cpu_gain)
