"""The recurrent population rollout (one GaussianGRUPolicy per env, rl_rollout_population_gru) and CEM / CMA-ES on it.

Parity evidence of the kind the fused rollouts have: the env dynamics replay bit for bit on the host build, the recorded
means sit within 1e-5 of the float64 scan (``dist_info_planes``) of each env's OWN candidate, and a candidate's columns are
bit for bit what the recurrent rollout (rl_rollout_gaussian_gru) records for that candidate."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CAND, N_EVALS, T, MPL = 35, 2, 25, 11          # 70 envs: a partial last wavefront, i % n_cand wraps inside the first
N = N_CAND * N_EVALS
PLANES = ("obs", "actions", "means", "rewards", "dones")


def _candidates(kind, hidden, include_action=True, n_cand=N_CAND, scale=0.1, seed=0):
    """(policy, xs float32 [n_cand, P] = theta + scale * randn per row -- h0, the biases and log_std too, so every lane has
    its own initial state and std --, kernel-layout rows on the device)."""
    from rllab_amd import _lib
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.spaces import Box
    q = _lib.env_query(kind)
    spec = EnvSpec(Box(-1e6 * np.ones(q["obs_dim"]), 1e6 * np.ones(q["obs_dim"])),
                   Box(-np.ones(q["act_dim"]), np.ones(q["act_dim"])))
    np.random.seed(seed)
    pol = GaussianGRUPolicy(spec, hidden_sizes=(hidden,), state_include_action=include_action)
    theta = pol.get_param_values()
    xs = (theta[None, :] + scale * np.random.RandomState(seed + 1).randn(n_cand, theta.size)).astype(np.float32)
    rows = pol.pack_rows(torch.as_tensor(xs, device=pol.flat_params.device))
    return pol, xs, rows


def _noise(q, n, horizon, seed=1):
    rng = np.random.RandomState(seed)
    eps = rng.randn(q["act_dim"], horizon, n).astype(np.float32)
    draws = (rng.randn if q["reset_is_normal"] else rng.rand)(horizon + 1, q["reset_draws"], n).astype(np.float32)
    return eps, draws


def _launch(v, pol, rows, horizon=T, n_evals=N_EVALS, discount=0.99, **kw):
    return v.rollout_population_recurrent(rows, n_evals, horizon, discount, pol.kernel_hidden, pol.state_include_action, **kw)


def _starts(traj):
    start = torch.ones_like(traj.dones, dtype=torch.bool)
    start[1:] = traj.dones[:-1].bool()
    return start


CASES = [(kind, hidden, True) for kind in (0, 2, 3) for hidden in (32, 20, 64)] + [(2, 32, False)]


@pytest.mark.parametrize("kind,hidden,include_action", CASES)
def test_population_gru_rollout_parity(kind, hidden, include_action):
    from rllab_amd.envs.hip_env import HipVecEnv
    from rllab_amd.sampler.trajectories import PathList
    from oracle.replay import replay_check
    pol, xs, rows = _candidates(kind, hidden, include_action)
    v = HipVecEnv(kind, N, MPL, normalize=True, seed=5)
    q = v.q
    eps, draws = _noise(q, N, T)
    traj, first_path = _launch(v, pol, rows, eps=eps, reset_draws=draws)
    assert v.step_counter == T + 1
    assert replay_check(v, traj, max_envs=N, reset_draws=draws) == N * T
    assert int(traj.dones.sum()) > 0
    # every env's means against the float64 scan of ITS candidate over the recorded planes (env i: candidate i % n_cand)
    start = _starts(traj)
    worst = 0.0
    for c in range(N_CAND):
        envs = [c + e * N_CAND for e in range(N_EVALS)]
        flat64 = torch.as_tensor(xs[c], device=traj.device).double()
        with torch.no_grad():
            d = pol.dist_info_planes(traj.obs[:, :, envs].double(), traj.actions[:, :, envs].double(), start[:, envs], flat64)
        worst = max(worst, float((traj.means[:, :, envs].double() - d["mean"]).abs().max()))
    print("population gru means vs float64, kind %d hidden %d include_action %s: max |diff| = %.3e" % (
        kind, hidden, include_action, worst))
    assert worst <= 1e-5
    # actions == means + eps * exp(log_std_c), the std in float32 (rounded once from float64), to within one float32 ulp
    da = q["act_dim"]
    std32 = np.exp(xs[:, -da:].astype(np.float64)).astype(np.float32)               # [n_cand, Da]
    std_env = np.tile(std32.T, (1, N_EVALS))[:, None, :].astype(np.float64)          # [Da, 1, n]
    act = traj.actions.cpu().numpy()
    want = traj.means.cpu().numpy().astype(np.float64) + eps.astype(np.float64) * std_env
    err_ulps = np.abs(act.astype(np.float64) - want) / np.spacing(np.abs(act)).astype(np.float64)
    print("actions vs means + eps * std: max %.3f ulp" % err_ulps.max())
    assert err_ulps.max() <= 1.0
    # the batch carries every env's own log_std row
    assert tuple(traj.log_std_planes.shape) == (da, T, N)
    assert np.array_equal(traj.log_std_planes[:, 3, :].cpu().numpy(), np.tile(xs[:, -da:].T, (1, N_EVALS)))
    # a path carries prev_action = its actions shifted by one step
    assert traj.prev_action_info == include_action
    path = PathList(traj)[1]
    if include_action:
        pa = path["agent_infos"]["prev_action"]
        assert np.all(pa[0] == 0) and np.array_equal(pa[1:], path["actions"][:-1])
    else:
        assert "prev_action" not in path["agent_infos"]


@pytest.mark.parametrize("injected", [False, True])
@pytest.mark.parametrize("kind,hidden", [(0, 32), (2, 20)])
def test_same_bits_as_the_recurrent_rollout(kind, hidden, injected):
    """Candidate c alone, as the policy of rl_rollout_gaussian_gru on a second executor of the same n, seed and step
    counter: columns c and c + N_CAND of all five planes are those of the population launch, bit for bit -- the shared
    cell's FMA order, the std, and the reset of h / prev_action to the candidate's own h0 / zeros."""
    from rllab_amd.envs.hip_env import HipVecEnv
    pol, xs, rows = _candidates(kind, hidden)
    v = HipVecEnv(kind, N, MPL, normalize=True, seed=5)
    kw = {}
    if injected:
        eps, draws = _noise(v.q, N, T)
        kw = dict(eps=eps, reset_draws=draws)
    traj, _ = _launch(v, pol, rows, **kw)
    assert int(traj.dones.sum()) > N                     # resets inside the launch
    for c in (0, 17, N_CAND - 1):
        pol.set_param_values(xs[c])
        assert np.array_equal(pol.get_param_values().astype(np.float32), xs[c])
        v2 = HipVecEnv(kind, N, MPL, normalize=True, seed=5)
        one = v2.rollout(pol, T, **kw)
        assert v2.step_counter == v.step_counter
        for name in PLANES:
            for col in (c, c + N_CAND):
                assert torch.equal(getattr(one, name)[..., col], getattr(traj, name)[..., col]), (name, c, col)
        # (and a column of another candidate is not: the candidates do differ)
        other = (c + 1) % N_CAND
        assert not torch.equal(one.means[..., other], traj.means[..., other])


def test_population_gru_candidate_mapping():
    """The same population with its rows permuted, the injected planes permuted the same way inside every evaluation
    block: every plane and first_path come out permuted identically, bit for bit."""
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 2
    pol, xs, rows = _candidates(kind, 32)
    q = HipVecEnv(kind, N, MPL, normalize=True, seed=5).q
    eps, draws = _noise(q, N, T)
    perm = np.random.RandomState(7).permutation(N_CAND)
    assert not np.array_equal(perm, np.arange(N_CAND))
    env_map = np.concatenate([e * N_CAND + perm for e in range(N_EVALS)])          # permuted env j runs original env_map[j]
    a, fa = _launch(HipVecEnv(kind, N, MPL, normalize=True, seed=5), pol, rows, eps=eps, reset_draws=draws)
    b, fb = _launch(HipVecEnv(kind, N, MPL, normalize=True, seed=5), pol, rows[torch.as_tensor(perm, device=rows.device)],
                    eps=eps[:, :, env_map], reset_draws=draws[:, :, env_map])
    idx = torch.as_tensor(env_map, device=rows.device)
    for name in PLANES:
        assert torch.equal(getattr(b, name), getattr(a, name)[..., idx]), name
    assert torch.equal(fb, fa[:, idx])
    assert not torch.equal(fb, fa)


# seed of the candidate draw and horizon below, chosen on the CPU so that at least a quarter of the 70 first paths end before
# the forced done and at least one does not: the test's own candidates (0.5 * randn around the seed's initial policy) and
# its own injected draws were replayed through the host env (oracle.host_env) with a numpy GRU, in float32 and in float64
# (tools/exp/population_gru_first_path_seed.py).  Under such perturbations a GRU drops the pole early: at a horizon of 100
# every path of seeds 0..39 ends before it, at 30 every path of seeds 0..5, at 20 two of seed 0 last, at 16 five of seed 0
# do -- 65 end early, in both precisions -- and between two and five of seeds 1..5.
FIRST_PATH_SEED, FIRST_PATH_HORIZON, FIRST_PATH_EARLY = 0, 16, 65


def test_first_path_accumulators_gru():
    from rllab_amd.envs.hip_env import HipVecEnv
    from oracle.replay import replay_check
    kind, horizon, gamma = 0, FIRST_PATH_HORIZON, 0.99
    pol, xs, rows = _candidates(kind, 32, scale=0.5, seed=FIRST_PATH_SEED)
    v = HipVecEnv(kind, N, horizon, normalize=True, seed=5)
    eps, draws = _noise(v.q, N, horizon)
    traj, first_path = _launch(v, pol, rows, horizon=horizon, discount=gamma, eps=eps, reset_draws=draws)
    done = traj.dones.cpu().numpy().astype(bool)
    rew = traj.rewards.cpu().numpy().astype(np.float64)
    fp = first_path.cpu().numpy()
    first_done = done.argmax(axis=0)                      # forced done at t = horizon - 1: every column has one
    assert done.any(axis=0).all()
    early = int((first_done < horizon - 1).sum())
    print("first paths: %d of %d envs end before T (CPU search: %r)" % (early, N, FIRST_PATH_EARLY))
    assert early >= N / 4 and early < N
    assert np.array_equal(fp[2], (first_done + 1).astype(np.float32))
    t = np.arange(horizon)[:, None]
    in_first = t <= first_done[None, :]
    disc_terms = np.where(in_first, gamma ** t * rew, 0.0)
    und_terms = np.where(in_first, rew, 0.0)
    bound = horizon * 2.0 ** -23
    err_d = np.abs(fp[0].astype(np.float64) - disc_terms.sum(axis=0))
    err_u = np.abs(fp[1].astype(np.float64) - und_terms.sum(axis=0))
    print("first-path returns: max err / bound = %.3e (discounted), %.3e (undiscounted)" % (
        (err_d / np.maximum(bound * np.abs(disc_terms).sum(axis=0), 1e-300)).max(),
        (err_u / np.maximum(bound * np.abs(und_terms).sum(axis=0), 1e-300)).max()))
    assert (err_d <= bound * np.abs(disc_terms).sum(axis=0)).all()
    assert (err_u <= bound * np.abs(und_terms).sum(axis=0)).all()
    # the envs keep running after the reset: every step, those after the first done included, replays on the host
    assert replay_check(v, traj, max_envs=N, reset_draws=draws) == N * horizon
    assert int(done.sum()) > N


def test_population_gru_philox_path():
    """No injected plane: the same seed and step_counter give the same planes, the next launch differs, and a launch
    that records nothing returns the same first_path."""
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 0
    pol, xs, rows = _candidates(kind, 32)
    va, vb, vc = (HipVecEnv(kind, N, MPL, normalize=True, seed=9) for _ in range(3))
    a, fa = _launch(va, pol, rows)
    b, fb = _launch(vb, pol, rows)
    for name in PLANES:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(fa, fb)
    a2, fa2 = _launch(va, pol, rows)
    assert va.step_counter == 2 * (T + 1)
    assert not torch.equal(a2.actions, a.actions) and not torch.equal(a2.obs, a.obs)
    none, fc = _launch(vc, pol, rows, record=False)
    assert none is None and torch.equal(fc, fa) and vc.step_counter == T + 1
    assert float(fa[2].min()) >= 1 and float(fa[2].max()) <= MPL


def test_population_gru_argument_errors_launch_nothing():
    from rllab_amd import _lib
    from rllab_amd.envs.hip_env import HipVecEnv
    lib = _lib.lib
    n_cand, horizon, H = 8, 3, 32
    v = HipVecEnv(0, n_cand, 5, normalize=True, seed=1)
    v.state.fill_(7)
    v.ts.fill_(7)
    dev = v.device
    theta_T = torch.zeros((8192, n_cand), dtype=torch.float32, device=dev)
    first_path = torch.full((3, n_cand), 7.0, dtype=torch.float32, device=dev)
    cfg = _lib.env_default_cfg(3, flags=_lib.CFG_CONTACT_MUJOCO)

    def call(**kw):
        a = dict(kind=0, n_cand=n_cand, n_evals=1, horizon=horizon, max_path_length=5, normalize=1, hidden=H,
                 include_action=1, env_offset=0, scale_reward=1.0, log_min_std=-1e30, discount=0.99, seed=1, step_counter=0,
                 state=v.state.data_ptr(), ts=v.ts.data_ptr(), theta_pop_T=theta_T.data_ptr(),
                 first_path=first_path.data_ptr())
        a.update(kw)
        return lib.rl_rollout_population_gru(ctypes.byref(_lib.PopulationGruArgs(**a)), None)

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.all(v.state == 7)) and bool(torch.all(v.ts == 7)) and bool(torch.all(first_path == 7))

    assert lib.rl_rollout_population_gru(None, None) == -1 and "null" in lib.rl_last_error().decode()
    for kw in (dict(theta_pop_T=None), dict(first_path=None), dict(include_action=2), dict(include_action=-1),
               dict(n_cand=0), dict(horizon=0), dict(state=None), dict(kind=99)):
        assert call(**kw) == -1 and lib.rl_last_error().decode(), kw
        assert untouched(), kw
    for hidden in (48, 128, 0):
        assert call(hidden=hidden) == -2 and "hidden = %d" % hidden in lib.rl_last_error().decode()
        assert untouched(), hidden
    assert call(kind=3, cfg=ctypes.pointer(cfg)) == -2 and "soft-constraint" in lib.rl_last_error().decode()
    assert untouched()


KEYS = ["Iteration", "CurStdMean", "AverageReturn", "StdReturn", "MaxReturn", "MinReturn", "AverageDiscountedReturn",
        "NumTrajs", "AvgTrajLen"]


def _train(tmp_path, name, algo):
    from rllab_amd.misc import logger
    path = str(tmp_path / (name + ".csv"))
    logger.add_tabular_output(path)
    try:
        algo.train()
    finally:
        logger.remove_tabular_output(path)
    with open(path) as f:
        reader = csv.DictReader(f)
        rows = list(reader)
        header = reader.fieldnames
    return header, rows


def _make(algo_name, hidden_sizes, seed=1, **kw):
    import importlib
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    ext.set_seed(seed)
    env = normalize(CartpoleEnv())
    policy = GaussianGRUPolicy(env_spec=env.spec, hidden_sizes=hidden_sizes)
    cls = getattr(importlib.import_module("rllab_amd.algos." + algo_name.lower().replace("cmaes", "cma_es")), algo_name)
    return cls(env=env, policy=policy, seed=seed, **kw), policy


def test_cem_end_to_end_with_a_gru(tmp_path, quiet_logger):
    kw = dict(n_itr=3, n_samples=70, max_path_length=100, n_evals=2, seed=1)
    algo, policy = _make("CEM", (32,), **kw)
    header, rows = _train(tmp_path, "a", algo)
    assert header[:len(KEYS)] == KEYS and header[len(KEYS):] == ["AveragePolicyStd"] and len(rows) == 3
    assert [int(r["Iteration"]) for r in rows] == [0, 1, 2]
    assert all(int(float(r["NumTrajs"])) == 70 for r in rows)
    assert all(np.isfinite(float(v)) for r in rows for v in r.values())
    # the policy holds the best candidate of the last iteration
    best = algo.last_xs[int(torch.sort(-algo.last_fs, stable=True).indices[0])]
    assert algo.last_xs.shape == (70, 3714)
    assert np.array_equal(policy.get_param_values().astype(np.float32), best.to(torch.float32).cpu().numpy())
    algo2, _ = _make("CEM", (32,), **kw)
    header2, rows2 = _train(tmp_path, "b", algo2)
    assert header2 == header and rows2 == rows


def test_cmaes_end_to_end_with_a_gru(tmp_path, quiet_logger):
    kw = dict(n_itr=3, max_path_length=100, seed=1)
    algo, policy = _make("CMAES", (8,), **kw)
    assert policy.get_param_values().size == 354
    header, rows = _train(tmp_path, "a", algo)
    assert len(rows) == 3 and "AveragePolicyStd" in header
    assert all(np.isfinite(float(v)) for r in rows for k, v in r.items() if k != "Stop")
    # every iteration's best candidate was told; the policy holds the best ever evaluated (what result()[0] is)
    assert len(algo.iteration_best) == 3
    i_best = int(torch.sort(algo.last_fs, stable=True).indices[0])
    assert torch.equal(algo.iteration_best[-1][1], algo.last_xs[i_best])
    assert np.array_equal(policy.get_param_values().astype(np.float32), algo.es.result()[0].to(torch.float32).cpu().numpy())
    f_best = min(float(f) for f, _ in algo.iteration_best)
    x_best = [x for f, x in algo.iteration_best if float(f) == f_best][0]
    assert np.array_equal(policy.get_param_values().astype(np.float32), x_best.to(torch.float32).cpu().numpy())
    algo2, _ = _make("CMAES", (8,), **kw)
    header2, rows2 = _train(tmp_path, "b", algo2)
    assert header2 == header and rows2 == rows


@pytest.mark.parametrize("case,word", [("hidden", "hidden_sizes=(100,)"), ("rectify", "rectify"),
                                       ("normalize_obs", "normalize_obs"), ("position_only", "position_only"),
                                       ("categorical", "GridWorldEnv is not a HIP-native env"), ("cmaes_size", "13570 parameters")])
def test_population_gru_refusals(case, word):
    from rllab_amd.algos.cem import CEM
    from rllab_amd.algos.cma_es import CMAES
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    cls = CMAES if case == "cmaes_size" else CEM
    if case == "categorical":
        from rllab_amd.envs.grid_world_env import GridWorldEnv
        from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
        env = GridWorldEnv()
        policy = CategoricalGRUPolicy(env_spec=env.spec)
    else:
        inner = CartpoleEnv(position_only=True) if case == "position_only" else CartpoleEnv()
        env = normalize(inner, normalize_obs=(case == "normalize_obs"))
        kw = dict(hidden=dict(hidden_sizes=(100,)), rectify=dict(hidden_nonlinearity=rectify),
                  cmaes_size=dict(hidden_sizes=(64,))).get(case, {})
        policy = GaussianGRUPolicy(env_spec=env.spec, **kw)
    with pytest.raises(NotImplementedError) as e:
        cls(env=env, policy=policy, n_itr=1, max_path_length=10).train()
    assert word in str(e.value), str(e.value)


# oracle: tools/exp/cem_gru_cpu_curves.py -- the same loop on the CPU (host env in float64, float64 numpy GRU, cem_scores /
# cem_refit) under examples/cem_gru_cartpole.py's CONFIG, seeds 1..5, committed as profiles/curves/cem_gru_cartpole_cpu.csv
LEARN_N_ITR = 7          # the smallest n_itr <= 20 at which all five CPU seeds gain
LEARN_MIN_CPU_GAIN = 5.9949717774372004   # (seed 4: 39.7 -> 45.7) the smallest gain of AverageReturn, iteration 0 -> iteration LEARN_N_ITR - 1, over the five seeds


def _cpu_gains(n_itr):
    curves = {}
    with open(os.path.join(ROOT, "profiles", "curves", "cem_gru_cartpole_cpu.csv")) as f:
        for r in csv.DictReader(f):
            curves.setdefault(int(r["Seed"]), {})[int(r["Iteration"])] = float(r["AverageReturn"])
    return {s: c[n_itr - 1] - c[0] for s, c in curves.items()}


def test_cem_learns_cartpole_with_a_gru(tmp_path, quiet_logger):
    """examples/cem_gru_cartpole.py's configuration, seed 1: AverageReturn must gain, from iteration 0 to the last, half of
    what the weakest of five CPU seeds gains over the same iterations -- half is the margin for the two samplers'
    different random streams."""
    from examples.cem_gru_cartpole import make_algo
    gains = _cpu_gains(LEARN_N_ITR)
    assert len(gains) == 5 and min(gains.values()) > 0 and LEARN_N_ITR <= 20
    assert abs(min(gains.values()) - LEARN_MIN_CPU_GAIN) <= 1e-6        # the number quoted above is the file's
    for n_itr in range(2, LEARN_N_ITR):
        assert min(_cpu_gains(n_itr).values()) <= 0, "a smaller n_itr at which every CPU seed gains: %d" % n_itr
    _, rows = _train(tmp_path, "learn", make_algo(seed=1, n_itr=LEARN_N_ITR, record_paths=False))
    gain = float(rows[-1]["AverageReturn"]) - float(rows[0]["AverageReturn"])
    print("CEM with a GRU on Cartpole: AverageReturn %s, gain %.2f (CPU seeds: min gain %.2f)" % (
        [round(float(r["AverageReturn"]), 1) for r in rows], gain, LEARN_MIN_CPU_GAIN))
    assert gain >= 0.5 * LEARN_MIN_CPU_GAIN
