"""The sampler's batch-size contract: ``obtain_samples`` returns AT LEAST ``batch_size`` samples in whole paths and
stops where the reference's lock-step loop stops (``while n_samples < self.algo.batch_size``,
sandbox/rocky/tf/samplers/vectorized_sampler.py:55; rllab/algos/batch_polopt.py:23-34,
rllab/sampler/parallel_sampler.py:98-126); ``whole_paths=False`` cuts the list to exactly ``batch_size`` samples
(``truncate_paths``, parallel_sampler.py:129-155).

The checker is the reference's OWN ``VectorizedSampler.obtain_samples`` (staged, unmodified) run over a replay of the
recorded batch (oracle/ref_vecsampler.py): it must consume exactly the lock steps the engine recorded -- one fewer and
the engine overshot, one more and the replay raises -- and return exactly the paths the engine lists.
"""
import importlib
import pickle
import types

import numpy as np
import pytest
import torch

from test_gpu_reference_vecenv import _check_fused_against_reference, _fused_setup, close
from test_ref_vecenv import draws_for, needs_ref

pytestmark = [pytest.mark.gpu, needs_ref]

ENVS = dict(cartpole=("rllab.envs.box2d.cartpole_env", "CartpoleEnv"),
            double_pendulum=("rllab.envs.box2d.double_pendulum_env", "DoublePendulumEnv"),
            swimmer=("rllab.envs.mujoco.swimmer_env", "SwimmerEnv"),
            hopper=("rllab.envs.mujoco.hopper_env", "HopperEnv"),
            walker=("rllab.envs.mujoco.walker2d_env", "Walker2DEnv"))


def make_algo(name, batch_size, T, n_envs=None, whole=True, hidden=(32, 32), norm=None, seed=3, **algo_kw):
    from rllab.algos.vpg import VPG
    from rllab.baselines.linear_feature_baseline import LinearFeatureBaseline
    from rllab.envs.normalized_env import normalize
    from rllab.misc import ext
    from rllab.policies.gaussian_mlp_policy import GaussianMLPPolicy
    ext.set_seed(seed)
    mod, cls = ENVS[name]
    env = normalize(getattr(importlib.import_module(mod), cls)(), **(norm or {}))
    pol = GaussianMLPPolicy(env_spec=env.spec, hidden_sizes=hidden)
    sampler_args = dict(seed=seed)
    if n_envs is not None:
        sampler_args["n_envs"] = n_envs
    algo = VPG(env=env, policy=pol, baseline=LinearFeatureBaseline(env_spec=env.spec), batch_size=batch_size,
               max_path_length=T, n_itr=1, whole_paths=whole, sampler_args=sampler_args, **algo_kw)
    algo.start_worker()
    algo.init_opt()
    return algo


def listed(paths):
    env, t0, t1 = (x.cpu().numpy() for x in paths.index())
    return sorted(zip(env.tolist(), t0.tolist(), (t1 - t0 + 1).tolist()))


def reference_loop(traj, batch_size, T, whole=True):
    from oracle import ref_vecsampler
    out = ref_vecsampler.run(traj.dones.cpu().numpy(), traj.rewards.cpu().numpy(), batch_size, T, whole)
    assert out["modules"]["sandbox.rocky.tf.samplers.vectorized_sampler"] == "sandbox/rocky/tf/samplers/vectorized_sampler.py"
    return out, sorted(zip(out["env"].tolist(), out["t0"].tolist(), out["length"].tolist()))


def check_contract(algo, batch_size, T, itr=0, paths=None):
    if paths is None:
        paths = algo.sampler.obtain_samples(itr)
    sd = algo.sampler.process_samples(0, paths)
    tr = paths.traj
    n_valid = int(tr.valid.sum())
    ref, ref_paths = reference_loop(tr, batch_size, T)
    assert int(ref["steps"]) == tr.T, "reference loop ran %d lock steps, the batch has %d" % (int(ref["steps"]), tr.T)
    assert listed(paths) == ref_paths
    assert n_valid == int(ref["length"].sum()) >= batch_size
    assert sd["observations"].shape[0] == n_valid and len(sd["paths"]) == len(ref_paths)
    env_i, _t0, t1 = paths.index()
    assert bool(tr.dones[t1, env_i].all())                     # every listed path ends in a done
    # reward sums per path, located through the reference's own bookkeeping
    got = {(e, a): float(tr.rewards[a:a + l, e].double().sum()) for e, a, l in listed(paths)}
    for e, a, s in zip(ref["env"], ref["t0"], ref["reward_sums"]):
        assert abs(got[(int(e), int(a))] - s) <= 1e-9 * max(1.0, abs(s))
    return paths, sd, ref


@pytest.mark.parametrize("name,batch_size,T,n_envs", [
    ("cartpole", 4000, 100, None),          # examples/trpo_cartpole.py's sizes: n_envs = 40
    ("cartpole", 4096 * 100, 100, 4096),    # BASELINE C2
    ("cartpole", 4000, 100, 512),           # far more envs than the batch needs: the loop stops after a few lock steps
    ("hopper", 6000, 60, 100),
    ("walker", 5000, 50, 100),              # the one-leg-per-lane rollout kernels carried on without a reset
])
def test_terminating_envs_return_at_least_batch_size_in_whole_paths(name, batch_size, T, n_envs, quiet_logger):
    algo = make_algo(name, batch_size, T, n_envs)
    assert algo.sampler.sampling_path(algo.policy)[0].startswith("fused rollout kernel")
    paths, sd, ref = check_contract(algo, batch_size, T)
    tr = paths.traj
    n = algo.sampler.vec_env.n
    assert batch_size <= int(tr.valid.sum()) < batch_size + n * T
    if n_envs == 512:
        assert tr.T < T
    theta0 = algo.policy.get_param_values()
    algo.optimize_policy(0, sd)
    assert np.abs(algo.policy.get_param_values() - theta0).max() > 0


def test_envs_that_never_terminate_stay_one_asynchronous_launch(quiet_logger, monkeypatch):
    """Swimmer (done always False): n_envs x max_path_length lock steps ARE batch_size whole-path samples; nothing is
    counted, nothing read back -- and the reference's loop agrees."""
    algo = make_algo("swimmer", 64 * 50, 50, 64)

    def boom(*a, **k):
        raise AssertionError("a never-terminating env's batch must not be counted on the host")
    monkeypatch.setattr(type(algo.sampler), "_finished_by_step", boom)
    paths, _sd, _ref = check_contract(algo, 64 * 50, 50)
    assert (paths.traj.T, paths.traj.N) == (50, 64) and len(paths) == 64


def test_fewer_envs_than_the_batch_needs_run_further_rounds(quiet_logger):
    """n_envs x max_path_length < batch_size (the reference caps n_envs at 100 and loops on,
    vectorized_sampler.py:22-24,55): further rounds on the same envs, no reset in between."""
    algo = make_algo("double_pendulum", 1000, 50, 8)
    paths, _sd, ref = check_contract(algo, 1000, 50)
    assert paths.traj.T == 150 and len(paths) == 24 and int(ref["length"].sum()) == 1200


@pytest.mark.parametrize("name,batch_size,T,n_envs", [("cartpole", 4000, 100, None), ("swimmer", 3000, 50, 64),
                                                      ("double_pendulum", 1000, 50, 8)])
def test_whole_paths_false_cuts_to_exactly_batch_size(name, batch_size, T, n_envs, quiet_logger):
    """``whole_paths=False``: the finished paths are collected as always, then the list -- in the order the paths
    finished -- is cut from its end to ``batch_size`` samples, the last kept path truncated.  The kept (env, t0, length)
    set is the one the reference's ``obtain_samples`` + ``truncate_paths`` keep on the same recording.  Cartpole: the
    cut falls mid-list; DoublePendulum never terminates: three rounds of 8 x 50 samples, the cut inside the third."""
    algo = make_algo(name, batch_size, T, n_envs, whole=False)
    recorded = []                              # the done flags before the cut marks the truncated path's new end
    keep_first = algo.sampler._keep_first

    def spy(traj, *a, **k):
        recorded.append(traj.dones.clone())
        return keep_first(traj, *a, **k)
    algo.sampler._keep_first = spy
    paths = algo.sampler.obtain_samples(0)
    sd = algo.sampler.process_samples(0, paths)
    tr = paths.traj
    assert len(recorded) == 1 and int(tr.valid.sum()) == batch_size == sd["observations"].shape[0]
    from oracle import ref_vecsampler
    ref = ref_vecsampler.run(recorded[0].cpu().numpy(), tr.rewards.cpu().numpy(), batch_size, T, False)
    assert int(ref["steps"]) == tr.T
    assert int(ref["length"].sum()) == batch_size
    assert listed(paths) == sorted(zip(ref["env"].tolist(), ref["t0"].tolist(), ref["length"].tolist()))
    if name == "double_pendulum":
        assert tr.T == 150 and int(tr.valid[:100].sum()) == 800 and int(tr.valid[100:].sum()) == 200
    algo.optimize_policy(0, sd)


@pytest.mark.parametrize("hidden,norm,loop", [((300,), None, "hipGraph replay"),
                                              ((100, 50, 25), dict(normalize_obs=True, normalize_reward=True), "eager")])
def test_per_transition_loops_meet_the_contract_too(hidden, norm, loop, quiet_logger):
    algo = make_algo("cartpole", 2000, 50, None, hidden=hidden, norm=norm)
    name, _why = algo.sampler.sampling_path(algo.policy)
    if not name.startswith("per-transition loop (%s)" % loop):
        pytest.skip("sampled by: %s" % name)                              # (a later round fused this shape)
    check_contract(algo, 2000, 50)


def test_running_normalisation_is_carried_over_the_further_launches(quiet_logger):
    """Fused rollout under NormalizedEnv(normalize_obs, normalize_reward): the continuation feeds every estimate once
    per transition -- the estimates after the batch are those of ONE stream of traj.T + 1 observations per env."""
    norm = dict(normalize_obs=True, normalize_reward=True, obs_alpha=0.01, reward_alpha=0.01)
    algo = make_algo("cartpole", 4000, 100, None, norm=norm)
    assert algo.sampler.sampling_path(algo.policy)[0].startswith("fused rollout kernel")
    paths, _sd, _ref = check_contract(algo, 4000, 100)
    assert paths.traj.T > 100                                             # the batch did need further launches


def test_dropped_speculative_batch_gives_its_rng_counter_back(quiet_logger):
    """A prefetched rollout whose parameters were then rejected is thrown away AND leaves no trace: the next batch is
    bit-identical to that of a run that never speculated."""
    runs = []
    for speculate in (True, False):
        algo = make_algo("swimmer", 32 * 20, 20, 32)
        algo.sampler.obtain_samples(0)
        theta = algo.policy.get_param_values()
        if speculate:
            algo.sampler.prefetch(1)
            assert algo.sampler._prefetched is not None
        algo.policy.set_param_values(theta * 0.5)                         # the step that was speculated on is reverted
        runs.append(algo.sampler.obtain_samples(1).traj)
    assert torch.equal(runs[0].obs, runs[1].obs) and torch.equal(runs[0].actions, runs[1].actions)


def test_running_normalisation_is_never_prefetched(quiet_logger):
    norm = dict(normalize_obs=True, normalize_reward=True)
    algo = make_algo("cartpole", 64 * 20, 20, 64, norm=norm)
    algo.sampler.obtain_samples(0)
    before = algo.sampler.vec_env.obs_mean.clone()
    algo.sampler.prefetch(1)
    assert getattr(algo.sampler, "_prefetched", None) is None
    assert torch.equal(before, algo.sampler.vec_env.obs_mean)


# -- what outlives the batch: NormalizedEnv's running estimates are those of the kept lock steps --------------------------
class DrawFeeder(object):
    """Which lock step of the current ``obtain_samples`` a launch / step starts at, from the executor's RNG counter: a
    launch that is taken back (the counter restored) and done again gets the slot it had, so every lock step sees the
    same slice of ONE pre-drawn table, as in test_fused_rollout_carried_on_without_a_reset_is_one_stream."""

    def __init__(self):
        self.seen, self.next, self.calls, self.redone = {}, 0, [], 0

    def slot(self, counter, steps, restart):
        if restart and counter not in self.seen:
            self.seen = {}
        t = 0 if restart else self.seen.get(counter, self.next)
        self.seen[counter] = t
        self.next = t + steps
        return t


def finished_by_step(dones):
    """n_samples of the reference's loop after every lock step of a recording (numpy)."""
    run, total, out = np.zeros(dones.shape[1], np.int64), 0, []
    for d in dones.astype(bool):
        run += 1
        total += int(run[d].sum())
        run[d] = 0
        out.append(total)
    return np.array(out)


@pytest.mark.parametrize("cut", ["first_launch", "continuation", "last_step"])
@pytest.mark.parametrize("name,n,mpl", [("cartpole", 96, 9), ("hopper", 48, 9)])
def test_estimates_after_obtain_samples_are_those_of_the_kept_lock_steps(name, n, mpl, cut, monkeypatch, quiet_logger):
    """Fused rollout under NormalizedEnv(normalize_obs, normalize_reward): the reference's loop stops stepping -- and
    feeding the running estimates -- at the lock step where n_samples >= batch_size.  After ``obtain_samples`` the
    executor's four estimate planes (and the observation it would carry on from) are those of the reference's executor
    fed the batch's first ``traj.T`` lock steps and no more, starting from non-trivial estimates; again after a second
    ``obtain_samples``; and the pickled env carries copy 0's.  batch_size is chosen from a probe run of the same stream
    so that the cut falls (a) inside the first launch of max_path_length steps, with many more envs than the batch
    needs, (b) inside a further launch, (c) on the first launch's last step.  A launch that is taken back and done
    again reproduces its kept steps bit for bit.
    max_path_length is 9, as in the tests the tolerance comes from (5e-5 / 5e-4 of _check_fused_against_reference): the
    policy's actions are not on the exact grid, the reference's action map is one rounding apart, and the dynamics
    amplify that along a path -- measured here with paths of up to 60 lock steps over two batches: 3.6e-4 (Cartpole)
    and 6.5e-4 (Hopper) on the whitened observations with every done flag equal."""
    from rllab_amd.sampler.vectorized_sampler import VectorizedSampler
    table = 4 * mpl + 16
    _env, pol, v, eps, draws, _est0 = _fused_setup(name, (True, True), "16", monkeypatch, table, n=n, mpl=mpl)
    F = finished_by_step(v.rollout(pol, 3 * mpl, eps=eps[:, :3 * mpl].copy(), reset_draws=draws[:3 * mpl + 1].copy())
                         .dones.cpu().numpy())
    if cut == "first_launch":
        assert F[mpl // 2] > 0, "no path of the probe ends in the first %d lock steps" % (mpl // 2)
        batch_size = int(F[np.nonzero(F)[0][0]])
    elif cut == "continuation":
        batch_size = int(F[mpl - 1]) + 1
    else:
        batch_size = int(F[mpl - 1])
        assert F[mpl - 1] > F[mpl - 2]
    stop = int(np.nonzero(F >= batch_size)[0][0]) + 1                          # lock steps the reference's loop takes
    print("%s %s: n_samples by step %s ..., batch_size %d, stop after %d" % (name, cut, F[:8].tolist(), batch_size, stop))

    env, pol, v, eps, draws, est0 = _fused_setup(name, (True, True), "16", monkeypatch, table, n=n, mpl=mpl)
    algo = types.SimpleNamespace(policy=pol, env=env, batch_size=batch_size, max_path_length=mpl, whole_paths=True)
    s = VectorizedSampler(algo, n_envs=n)
    s.vec_env = v
    feed = DrawFeeder()
    feed.eps, feed.draws = eps, draws
    rollout = v.rollout

    def fed(policy, steps, reset_at_start=True):
        t = feed.slot(v.inner.step_counter, steps, reset_at_start)
        assert t + steps <= table
        out = rollout(policy, steps, reset_at_start=reset_at_start, eps=feed.eps[:, t:t + steps].copy(),
                      reset_draws=feed.draws[t:t + steps + 1].copy())
        if feed.calls and feed.calls[-1][0] == t and steps < feed.calls[-1][1]:
            prev = feed.calls[-1][2]                                          # the launch this one does again, shorter
            for plane in ("obs", "actions", "means"):
                assert torch.equal(getattr(out, plane), getattr(prev, plane)[:, :steps]), plane
            assert torch.equal(out.rewards, prev.rewards[:steps]) and torch.equal(out.dones, prev.dones[:steps])
            feed.redone += 1
        feed.calls.append((t, steps, out))
        return out
    v.rollout = fed

    before = None
    for itr in (0, 1):
        traj = s.obtain_samples(itr).traj
        launches = [(t, k) for t, k, _ in feed.calls]
        print("itr %d: %d lock steps, launches (from, steps) %s, redone %d" % (itr, traj.T, launches, feed.redone))
        if itr == 0:
            assert traj.T == stop
            if cut == "first_launch":
                assert traj.T < mpl and launches == [(0, mpl), (0, traj.T)] and feed.redone == 1
            elif cut == "continuation":
                assert traj.T > mpl and feed.redone == 1 and launches[-1] == (launches[-2][0], traj.T - launches[-2][0])
            else:
                assert traj.T == mpl and launches == [(0, mpl)] and feed.redone == 0
        ref = _check_fused_against_reference(name, v, traj, feed.draws[:traj.T + 1], est0, mpl, min_dones=1, before=before)
        tol = 5e-4 if name == "hopper" else 5e-5
        clone = pickle.loads(pickle.dumps(env))
        for got, want in ((clone._obs_stats.mean, ref["obs_mean"][0]), (clone._obs_stats.var, ref["obs_var"][0])):
            ok, err = close(got, want, tol)
            assert ok, err
        # the next obtain_samples goes on from these estimates on the same env copies (its reset feeds the estimates once
        # more, in the reference too), on a fresh table: the reference's executor runs both batches, from est0
        before = (traj.actions.permute(1, 2, 0).cpu().numpy(), feed.draws[:traj.T + 1])
        rng = np.random.RandomState(11)
        feed.eps = rng.randn(v.q["act_dim"], table, n).astype(np.float32)
        feed.draws = draws_for(v.q, rng, table, n)
        feed.calls, feed.redone = [], 0


def test_estimates_after_obtain_samples_on_the_eager_loop(quiet_logger):
    """The per-transition loop (eager: the executor under running normalisation is not graphable) steps through
    ``NormalizingVecEnv.step``; a launch that ran past the cut is taken back and the envs are stepped through the
    recorded actions of the kept lock steps.  Estimates against the reference's executor fed ``traj.T`` lock steps,
    within rtol 1e-12 / atol 1e-14: the policy's actions are put on the 1/64 grid that makes NormalizedEnv's action map
    exact (tests/test_ref_vecenv.py::grid_actions), so the raw streams are bit-identical."""
    from oracle import ref_vecenv
    T, n = 100, 256
    norm = dict(normalize_obs=True, normalize_reward=True, obs_alpha=0.01, reward_alpha=0.02)
    algo = make_algo("cartpole", 600, T, n, hidden=(100, 50, 25), norm=norm)
    s, pol = algo.sampler, algo.policy
    assert s.sampling_path(pol)[0].startswith("per-transition loop (eager)")
    v = s.vec_env
    rng = np.random.RandomState(2)
    v.obs_mean += torch.as_tensor(0.1 * rng.randn(v.q["obs_dim"], n), device=v.obs_mean.device)
    v.reward_var *= 1.5
    get_actions = pol.get_actions

    def gridded(obs):
        a, info = get_actions(obs)
        return torch.clamp(torch.round(a * 64.0) / 64.0, -1.5, 1.5), info
    pol.get_actions = gridded
    feed = DrawFeeder()
    reset, step, stepped = v.reset, v.step, []

    def fed_reset():
        feed.slot(v.inner.step_counter, 0, True)
        return reset(draws=feed.draws[0])

    def fed_step(actions):
        t = feed.slot(v.inner.step_counter, 1, False)
        stepped.append(t)
        return step(actions, reset_draws=feed.draws[t + 1])
    v.reset, v.step = fed_reset, fed_step
    est0 = dict(obs_mean0=v.obs_mean.t().cpu().numpy(), obs_var0=v.obs_var.t().cpu().numpy(),
                reward_mean0=v.reward_mean.cpu().numpy(), reward_var0=v.reward_var.cpu().numpy())
    done_a, done_d = [], []                    # actions and draws of the batches so far: the reference's executor runs them
    for itr in (0, 1):                         # all, on the same env copies, with a reset of its own before each
        feed.draws = draws_for(v.q, np.random.RandomState(20 + itr), 4 * T, n)
        del stepped[:]
        traj = s.obtain_samples(itr).traj
        print("itr %d: %d lock steps kept, %d stepped" % (itr, traj.T, len(stepped)))
        # the launch ran past the cut and its kept steps were stepped again
        assert max(stepped) + 1 > traj.T and stepped[-1] == traj.T - 1 and len(stepped) > max(stepped) + 1
        done_a.append(traj.actions.permute(1, 2, 0).cpu().numpy())
        done_d.append(feed.draws[:traj.T + 1])
        T0 = sum(a.shape[0] for a in done_a[:-1])
        ref = ref_vecenv.run(v.kind, T, np.concatenate(done_a), np.concatenate(done_d), reset_at=[T0] if itr else (),
                             **dict(norm, **est0))
        assert np.array_equal(traj.dones.cpu().numpy().astype(bool), ref["dones"][T0:])
        kw = dict(rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(v.obs_mean.t().cpu().numpy(), ref["obs_mean"], **kw)
        np.testing.assert_allclose(v.obs_var.t().cpu().numpy(), ref["obs_var"], **kw)
        np.testing.assert_allclose(v.reward_mean.cpu().numpy(), ref["reward_mean"], **kw)
        np.testing.assert_allclose(v.reward_var.cpu().numpy(), ref["reward_var"], **kw)
        clone = pickle.loads(pickle.dumps(algo.env))
        np.testing.assert_allclose(clone._obs_stats.mean, ref["obs_mean"][0], **kw)
        np.testing.assert_allclose(clone._obs_stats.var, ref["obs_var"][0], **kw)


def test_hip_graph_loop_has_no_estimates_to_carry_and_meets_the_contract_twice(quiet_logger):
    """The hipGraph replay of the per-transition loop only ever runs on a plain executor (running normalisation makes an
    executor non-graphable: the eager loop above): there is nothing a launch past the cut could leave behind, and the
    batch of a second ``obtain_samples`` is cut where the reference's loop stops, like the first."""
    algo = make_algo("cartpole", 2000, 50, None, hidden=(300,))
    name, _why = algo.sampler.sampling_path(algo.policy)
    if not name.startswith("per-transition loop (hipGraph replay)"):
        pytest.skip("sampled by: %s" % name)                              # (a later round fused this shape)
    assert not getattr(algo.sampler.vec_env, "stateful_rollouts", False)
    check_contract(algo, 2000, 50, itr=0)
    check_contract(algo, 2000, 50, itr=1)
    norm = make_algo("cartpole", 2000, 50, None, hidden=(300,), norm=dict(normalize_obs=True))
    assert norm.sampler.sampling_path(norm.policy)[0].startswith("per-transition loop (eager)")


# -- long batches on few envs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_envs,T,batch_size", [("cartpole", 1, 5, 3000), ("cartpole", 4, 10, 4000),
                                                      ("hopper", 4, 5, 3000), ("hopper", 1, 10, 2000)])
def test_long_batches_on_few_envs(name, n_envs, T, batch_size, quiet_logger, monkeypatch):
    """batch_size well beyond 65 * n_envs * max_path_length: the reference just keeps looping.  The sampler keeps
    launching while paths finish; every launch is scanned on its own (its lock steps and no others) with one host read,
    whatever the number of launches before it."""
    assert batch_size > 65 * n_envs * T
    algo = make_algo(name, batch_size, T, n_envs)
    s = algo.sampler
    scans, launches, reads = [], [], []
    by_step, chunk, to_host = s._finished_by_step, s._rollout_chunk, torch.Tensor.cpu

    def counted_scan(traj, *a, **k):
        scans.append(traj.T)
        return by_step(traj, *a, **k)

    def counted_chunk(policy, steps, first):
        out = chunk(policy, steps, first)
        launches.append(out.T)
        return out

    def counted_cpu(t, *a, **k):
        if t.is_cuda:
            reads.append(t.numel())
        return to_host(t, *a, **k)
    s._finished_by_step, s._rollout_chunk = counted_scan, counted_chunk
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", counted_cpu)
        paths = s.obtain_samples(0)
    print("launches %s, scans %s, reads %s" % (launches, scans, reads))
    assert scans == launches and reads == launches            # one scan and one read of [steps] counts per launch
    assert sum(launches) >= paths.traj.T > 65 * T
    check_contract(algo, batch_size, T, paths=paths)
