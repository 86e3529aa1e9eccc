"""The population rollout (one parameter vector per env, rl_rollout_population) and CEM on it (rllab/algos/cem.py).

Parity evidence of the kind the fused rollouts have: the env dynamics replay bit for bit on the host build, the recorded
means sit within 1e-5 of the float64 forward pass of each env's OWN candidate."""
import csv
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CAND, N_EVALS, T = 35, 2, 25          # 70 envs: a partial last wavefront


def _candidates(kind, hidden, n_cand=N_CAND, scale=0.1, seed=0):
    """(policy, xs float32 [n_cand, P] = theta + scale * randn per row -- the log_std entries too, so every lane has its
    own std --, kernel-layout rows on the device)."""
    from tests.test_gpu_env_parity import _make_policy
    pol = _make_policy(kind, hidden, seed)
    theta = pol.get_param_values()
    xs = (theta[None, :] + scale * np.random.RandomState(seed + 1).randn(n_cand, theta.size)).astype(np.float32)
    lay = pol.kernel_layout()
    assert lay is not None and not lay.wide
    rows = lay.pack_rows(torch.as_tensor(xs, device=pol.flat_params.device))
    return pol, xs, rows


def _noise(q, n, horizon, seed=1):
    rng = np.random.RandomState(seed)
    eps = rng.randn(q["act_dim"], horizon, n).astype(np.float32)
    draws = (rng.randn if q["reset_is_normal"] else rng.rand)(horizon + 1, q["reset_draws"], n).astype(np.float32)
    return eps, draws


def _launch(v, pol, rows, horizon=T, n_evals=N_EVALS, discount=0.99, **kw):
    return v.rollout_population(rows, n_evals, horizon, discount, layer_activations=pol.kernel_layout().layer_activations,
                                log_min_std=math.log(pol.min_std), **kw)


@pytest.mark.parametrize("hidden", [(32, 32), (20, 20), (64, 64), (20,)])
@pytest.mark.parametrize("kind", [0, 2, 3])
def test_population_rollout_parity(kind, hidden):
    from rllab_amd.envs.hip_env import HipVecEnv
    from oracle.replay import replay_check
    pol, xs, rows = _candidates(kind, hidden)
    n = N_CAND * N_EVALS
    v = HipVecEnv(kind, n, 11, normalize=True, seed=5)
    q = v.q
    eps, draws = _noise(q, n, T)
    traj, first_path = _launch(v, pol, rows, eps=eps, reset_draws=draws)
    assert v.step_counter == T + 1
    assert replay_check(v, traj, max_envs=n, reset_draws=draws) == n * T
    assert int(traj.dones.sum()) > 0
    # every env's means against the float64 forward pass of ITS candidate (env i: candidate i % n_cand)
    worst = 0.0
    for c in range(N_CAND):
        envs = [c + e * N_CAND for e in range(N_EVALS)]
        obs64 = traj.obs[:, :, envs].reshape(q["obs_dim"], -1).double()
        with torch.no_grad():
            mean64 = pol.mean_planes(obs64, torch.as_tensor(xs[c], device=obs64.device).double())
        got = traj.means[:, :, envs].reshape(q["act_dim"], -1).double()
        worst = max(worst, float((got - mean64).abs().max()))
    print("population means vs float64, kind %d hidden %r: max |diff| = %.3e" % (kind, hidden, worst))
    assert worst <= 1e-5
    # actions == means + eps * exp(max(log_std_c, log_min_std)), the std in the policy's float32 (rounded once from
    # float64), to within one float32 ulp of the action (the kernel's one fma rounds once: half an ulp)
    ls = xs[:, -q["act_dim"]:].astype(np.float64)                                  # [n_cand, Da]
    std32 = np.exp(np.maximum(ls, math.log(pol.min_std))).astype(np.float32)
    std_env = np.tile(std32.T, (1, N_EVALS))[:, None, :].astype(np.float64)         # [Da, 1, n]
    act = traj.actions.cpu().numpy()
    want = traj.means.cpu().numpy().astype(np.float64) + eps.astype(np.float64) * std_env
    err_ulps = np.abs(act.astype(np.float64) - want) / np.spacing(np.abs(act)).astype(np.float64)
    print("actions vs means + eps * std: max %.3f ulp" % err_ulps.max())
    assert err_ulps.max() <= 1.0
    # and the batch carries every env's own log_std
    assert tuple(traj.log_std_planes.shape) == (q["act_dim"], T, n)
    want_ls = np.tile(np.maximum(xs[:, -q["act_dim"]:], np.float32(math.log(pol.min_std))).T, (1, N_EVALS))
    assert np.array_equal(traj.log_std_planes[:, 3, :].cpu().numpy(), want_ls)


@pytest.mark.parametrize("kind", [0, 2])
def test_population_rollout_with_env_noise(kind):
    """Box2DEnv / MujocoEnv(action_noise=.., obs_noise=..) inside the population rollout: the injected N(0,1) planes of
    both noises reach the step and the observation exactly as in the fused rollout -- the host replays bit for bit."""
    from rllab_amd.envs.hip_env import HipVecEnv
    from oracle.replay import replay_check
    pol, xs, rows = _candidates(kind, (32, 32))
    n = N_CAND * N_EVALS
    cfg = dict(action_noise=0.1, obs_noise=0.05) if kind == 0 else dict(action_noise=0.1)
    v = HipVecEnv(kind, n, 11, normalize=True, seed=5, cfg=cfg)
    q = v.q
    eps, draws = _noise(q, n, T)
    rng = np.random.RandomState(3)
    az = rng.randn(T, q["act_dim"], n).astype(np.float32)
    oz = rng.randn(T + 1, q["obs_dim"], n).astype(np.float32)
    traj, _ = _launch(v, pol, rows, eps=eps, reset_draws=draws, action_noise_z=az, obs_noise_z=oz)
    assert replay_check(v, traj, max_envs=n, reset_draws=draws, action_noise_z=az, obs_noise_z=oz) == n * T


def test_population_candidate_mapping():
    """The same population with its rows permuted, the injected planes permuted the same way inside every evaluation
    block: every plane and first_path come out permuted identically, bit for bit."""
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 2
    pol, xs, rows = _candidates(kind, (32, 32))
    n = N_CAND * N_EVALS
    q = HipVecEnv(kind, n, 11, normalize=True, seed=5).q
    eps, draws = _noise(q, n, T)
    perm = np.random.RandomState(7).permutation(N_CAND)
    assert not np.array_equal(perm, np.arange(N_CAND))
    env_map = np.concatenate([e * N_CAND + perm for e in range(N_EVALS)])          # permuted env j runs original env_map[j]
    a, fa = _launch(HipVecEnv(kind, n, 11, normalize=True, seed=5), pol, rows, eps=eps, reset_draws=draws)
    b, fb = _launch(HipVecEnv(kind, n, 11, normalize=True, seed=5), pol, rows[torch.as_tensor(perm, device=rows.device)],
                    eps=eps[:, :, env_map], reset_draws=draws[:, :, env_map])
    idx = torch.as_tensor(env_map, device=rows.device)
    for name in ("obs", "actions", "means", "rewards", "dones"):
        assert torch.equal(getattr(b, name), getattr(a, name)[..., idx]), name
    assert torch.equal(fb, fa[:, idx])
    assert not torch.equal(fb, fa)


# seed of the candidate draw below, chosen so that at least a quarter of the 70 envs terminate before T and one does not:
# under 0.5 * randn perturbations nearly every candidate drops the pole within 60 steps; of seeds 0..599 only this one has a
# candidate (24) that holds it for 100 steps in both of its evaluations, found by replaying the test's own draws through the
# host env (oracle.host_env) with a numpy policy, in float32 and float64 alike
FIRST_PATH_SEED = 402


def test_first_path_accumulators():
    from rllab_amd.envs.hip_env import HipVecEnv
    from oracle.replay import replay_check
    kind, horizon, gamma = 0, 100, 0.99
    pol, xs, rows = _candidates(kind, (32, 32), scale=0.5, seed=FIRST_PATH_SEED)
    n = N_CAND * N_EVALS
    v = HipVecEnv(kind, n, horizon, normalize=True, seed=5)
    eps, draws = _noise(v.q, n, horizon)
    traj, first_path = _launch(v, pol, rows, horizon=horizon, discount=gamma, eps=eps, reset_draws=draws)
    done = traj.dones.cpu().numpy().astype(bool)
    rew = traj.rewards.cpu().numpy().astype(np.float64)
    fp = first_path.cpu().numpy()
    first_done = done.argmax(axis=0)                      # forced done at t = horizon - 1: every column has one
    assert done.any(axis=0).all()
    early = int((first_done < horizon - 1).sum())
    print("first paths: %d of %d envs end before T" % (early, n))
    assert early >= n / 4 and early < n
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
    assert replay_check(v, traj, max_envs=n, reset_draws=draws) == n * horizon
    assert int(done.sum()) > n


def test_population_philox_path():
    """No injected plane: the same seed and step_counter give the same planes, the next launch differs, and a launch
    that records nothing returns the same first_path."""
    from rllab_amd.envs.hip_env import HipVecEnv
    kind = 0
    pol, xs, rows = _candidates(kind, (32, 32))
    n = N_CAND * N_EVALS
    va, vb, vc = (HipVecEnv(kind, n, 11, normalize=True, seed=9) for _ in range(3))
    a, fa = _launch(va, pol, rows)
    b, fb = _launch(vb, pol, rows)
    for name in ("obs", "actions", "means", "rewards", "dones"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(fa, fb)
    a2, fa2 = _launch(va, pol, rows)
    assert not torch.equal(a2.actions, a.actions) and not torch.equal(a2.obs, a.obs)
    none, fc = _launch(vc, pol, rows, record=False)
    assert none is None and torch.equal(fc, fa)
    assert float(fa[2].min()) >= 1 and float(fa[2].max()) <= 11


KEYS = ["Iteration", "CurStdMean", "AverageReturn", "StdReturn", "MaxReturn", "MinReturn", "AverageDiscountedReturn",
        "NumTrajs", "AvgTrajLen"]


def _train(tmp_path, name, snapshot=False, **kw):
    from rllab_amd.algos.cem import CEM
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.misc import ext, logger
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(kw.get("seed", 1))
    env = normalize(CartpoleEnv())
    policy = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=(32, 32))
    algo = CEM(env=env, policy=policy, **kw)
    path = str(tmp_path / (name + ".csv"))
    old_dir, old_mode = logger.get_snapshot_dir(), logger.get_snapshot_mode()
    logger.add_tabular_output(path)
    if snapshot:
        logger.set_snapshot_dir(str(tmp_path))
        logger.set_snapshot_mode("last")
    try:
        algo.train()
    finally:
        logger.remove_tabular_output(path)
        logger.set_snapshot_dir(old_dir)
        logger.set_snapshot_mode(old_mode)
    with open(path) as f:
        reader = csv.DictReader(f)
        rows = list(reader)
        header = reader.fieldnames
    return algo, policy, header, rows


def test_cem_end_to_end(tmp_path, quiet_logger):
    kw = dict(n_itr=3, n_samples=70, max_path_length=100, n_evals=2, seed=1)
    algo, policy, header, rows = _train(tmp_path, "a", snapshot=True, **kw)
    assert header[:len(KEYS)] == KEYS and len(rows) == 3
    assert [int(r["Iteration"]) for r in rows] == [0, 1, 2]
    assert all(int(float(r["NumTrajs"])) == 70 for r in rows)
    assert "AveragePolicyStd" in header                          # policy.log_diagnostics ran on the first paths
    # the policy holds the best candidate of the last iteration
    best = algo.last_xs[int(torch.sort(-algo.last_fs, stable=True).indices[0])]
    assert np.array_equal(policy.get_param_values().astype(np.float32), best.to(torch.float32).cpu().numpy())
    import joblib
    snap = joblib.load(str(tmp_path / "params.pkl"))
    assert snap["itr"] == 2 and snap["cur_mean"].shape == snap["cur_std"].shape == (policy.get_param_values().size,)
    assert abs(float(np.mean(snap["cur_std"])) - float(rows[-1]["CurStdMean"])) <= 1e-9
    _, _, header2, rows2 = _train(tmp_path, "b", **kw)
    assert header2 == header and rows2 == rows


# oracle: tools/exp/cem_cpu_curves.py -- the same loop on the CPU (host env in float64, float64 numpy policy, cem_scores /
# cem_refit), seeds 1..5, committed as profiles/curves/cem_cartpole_cpu.csv
LEARN_N_ITR = 7          # the smallest n_itr at which all five CPU seeds gain
LEARN_MIN_CPU_GAIN = 10.986785417998831   # (seed 4: 51.4 -> 62.4) the smallest gain of AverageReturn, iteration 0 -> iteration LEARN_N_ITR - 1, over the five seeds


def _cpu_gains(n_itr):
    curves = {}
    with open(os.path.join(ROOT, "profiles", "curves", "cem_cartpole_cpu.csv")) as f:
        for r in csv.DictReader(f):
            curves.setdefault(int(r["Seed"]), {})[int(r["Iteration"])] = float(r["AverageReturn"])
    return {s: c[n_itr - 1] - c[0] for s, c in curves.items()}


def test_cem_learns_cartpole(tmp_path, quiet_logger):
    """The reference's defaults (n_samples=100, max_path_length=500, ...) on Cartpole: AverageReturn must gain, from iteration
    0 to the last, half of what the weakest of five CPU seeds gains over the same iterations."""
    gains = _cpu_gains(LEARN_N_ITR)
    assert len(gains) == 5 and min(gains.values()) > 0
    assert abs(min(gains.values()) - LEARN_MIN_CPU_GAIN) <= 1e-6        # the number quoted above is the file's
    for n_itr in range(2, LEARN_N_ITR):
        assert min(_cpu_gains(n_itr).values()) <= 0, "a smaller n_itr at which every CPU seed gains: %d" % n_itr
    _, _, _, rows = _train(tmp_path, "learn", n_itr=LEARN_N_ITR, n_samples=100, seed=1, record_paths=False)
    gain = float(rows[-1]["AverageReturn"]) - float(rows[0]["AverageReturn"])
    print("CEM on Cartpole: AverageReturn %s, gain %.2f (CPU seeds: min gain %.2f)" % (
        [round(float(r["AverageReturn"]), 1) for r in rows], gain, LEARN_MIN_CPU_GAIN))
    assert gain >= 0.5 * LEARN_MIN_CPU_GAIN


def test_cem_batch_size_criterion(tmp_path, quiet_logger):
    """batch_size=1500, max_path_length=100: launches of 15 candidates until the counted lengths reach 1500; the population
    is the prefix rule applied to the recorded lengths."""
    from rllab_amd.algos.cem import cem_sample_prefix
    algo, _, _, rows = _train(tmp_path, "bs", n_itr=2, batch_size=1500, max_path_length=100, n_samples=100, seed=3)
    lengths = algo.last_lengths.cpu().numpy()              # length of the LAST evaluation's path of every candidate launched
    assert lengths.size % 15 == 0 and lengths.size >= 15
    used = cem_sample_prefix(lengths, 1500)
    assert used is not None and cem_sample_prefix(lengths[:lengths.size - 15], 1500) is None     # no launch too many
    assert int(float(rows[-1]["NumTrajs"])) == used == algo.last_n_candidates == algo.last_xs.shape[0]
    assert lengths[:used].sum() >= 1500 > lengths[:used - 1].sum()
    print("batch_size criterion: %d candidates launched, %d used" % (lengths.size, used))


@pytest.mark.parametrize("case,word", [("wide", "hidden_sizes"), ("rectify", "rectify"), ("adaptive_std", "adaptive_std"),
                                       ("normalize_obs", "normalize_obs")])
def test_cem_refusals(case, word):
    from rllab_amd.algos.cem import CEM
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
    env = normalize(CartpoleEnv(), normalize_obs=(case == "normalize_obs"))
    kw = dict(wide=dict(hidden_sizes=(100, 50, 25)), rectify=dict(hidden_nonlinearity=rectify),
              adaptive_std=dict(adaptive_std=True), normalize_obs=dict())[case]
    policy = GaussianMLPPolicy(env_spec=env.spec, **kw)
    with pytest.raises(NotImplementedError) as e:
        CEM(env=env, policy=policy, n_itr=1, n_samples=8, max_path_length=10).train()
    assert word in str(e.value), str(e.value)
