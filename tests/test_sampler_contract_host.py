"""Host-side pieces of the sampler's batch-size contract (CPU): the replay harness around the reference's OWN
``VectorizedSampler.obtain_samples`` / ``truncate_paths`` (oracle/ref_vecsampler.py) on a hand-checkable recording, and
``VectorizedSampler._keep_first`` (``whole_paths=False``) against what ``truncate_paths`` leaves of the same paths listed
in the reference's order (by the lock step a path ends at, then by env), and the extension loop ``_meet_batch_size`` on
stub launches: the reference's recorded answers, long batches on few envs, and a batch that cannot finish."""
import numpy as np
import pytest
import torch

from golden_util import ref_run
from test_ref_vecenv import HAVE_REF


def recording():
    # env 0: paths end at t = 1 and t = 4; env 1: at t = 2 and t = 5
    d = np.zeros((6, 2), np.uint8)
    d[1, 0] = d[4, 0] = d[2, 1] = d[5, 1] = 1
    return d, np.arange(12.0).reshape(6, 2)


# (batch size asked for, whole_paths, lock steps the loop takes, paths it keeps as (env, t0, length)); the reference
# loop's answers are recorded in tests/golden/ref_runs.npz (oracle/make_golden_refruns.py) and re-run live where the
# reference is staged
LOOP_CASES = [
    (2, True, 2, [(0, 0, 2)]),
    (3, True, 3, [(0, 0, 2), (1, 0, 3)]),
    (3, False, 3, [(0, 0, 2), (1, 0, 1)]),
    (6, True, 5, [(0, 0, 2), (1, 0, 3), (0, 2, 3)]),
    (6, False, 5, [(0, 0, 2), (1, 0, 3), (0, 2, 1)]),
    (11, True, 6, [(0, 0, 2), (1, 0, 3), (0, 2, 3), (1, 3, 3)]),
]


def loop_case_name(want, whole):
    return "vec_sampler_loop_%d_%s" % (want, "whole" if whole else "cut")


def loop_reference(want, whole):
    from oracle import ref_vecsampler
    d, r = recording()
    return ref_vecsampler.run(d, r, want, 100, whole)


@pytest.mark.parametrize("want,whole,steps,paths", LOOP_CASES)
def test_reference_loop_on_a_replayed_recording(want, whole, steps, paths):
    out = ref_run(loop_case_name(want, whole), (lambda: loop_reference(want, whole)) if HAVE_REF else None)
    assert int(out["steps"]) == steps
    assert list(zip(out["env"].tolist(), out["t0"].tolist(), out["length"].tolist())) == paths


def test_reference_loop_refuses_a_recording_that_is_too_short():
    rec = ref_run("vec_sampler_loop_too_short")        # what the reference's loop said, recorded
    assert "asks for lock step 6" in str(rec["error"])
    if HAVE_REF:
        with pytest.raises(RuntimeError, match="asks for lock step 6"):
            loop_reference(12, True)


def completion_order(tr, whole):
    """The finished paths of ``tr`` as the reference's loop lists them: a path is appended at the lock step it ends at,
    envs in index order within a lock step (vectorized_sampler.py:72-97).  Path dicts hold the rewards only."""
    from rllab_amd.sampler.trajectories import PathList
    tr.valid = whole
    paths = PathList(tr)
    env, _t0, t1 = (x.numpy() for x in paths.index())
    order = np.lexsort((env, t1))                                      # by end lock step, then by env
    return [dict(rewards=paths[int(i)]["rewards"]) for i in order]


def check_against_truncate_paths(make, whole, want):
    """``_keep_first`` on a fresh copy of the batch against ``truncate_paths`` (the product's copy, pinned to the
    reference's by tests/test_reference_tests_verbatim.py) applied to the paths in completion order.  Rewards are
    distinct numbers, so a path is identified by its rewards."""
    from rllab_amd.sampler.trajectories import PathList
    from rllab_amd.sampler.utils import truncate_paths
    from rllab_amd.sampler.vectorized_sampler import VectorizedSampler
    base = make()
    full = completion_order(base, base.valid_mask(True) if whole is None else whole)
    tr = make()
    VectorizedSampler._keep_first(tr, want, whole)
    assert int(tr.valid.sum()) == want
    got = sorted(tuple(p["rewards"].tolist()) for p in PathList(tr))
    ref = sorted(tuple(p["rewards"].tolist()) for p in truncate_paths(full, want))
    assert got == ref
    return tr


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_keep_first_is_truncate_paths_in_completion_order(seed):
    from rllab_amd.sampler.trajectories import Trajectories
    rng = np.random.RandomState(seed)
    T, N = 23, 7
    dones = torch.as_tensor((rng.rand(T, N) < 0.15).astype(np.uint8))
    rewards = torch.as_tensor(rng.randn(T, N).astype(np.float32))
    z3 = lambda d, t=T: torch.zeros((d, t, N))
    make = lambda: Trajectories(z3(2), z3(1), z3(1), torch.zeros(1), rewards, dones.clone(), T)
    whole = make().valid_mask(True)
    total = int(whole.sum())
    assert len(set(rewards.reshape(-1).tolist())) == T * N
    for want in (1, total // 3, total // 2, total - 1, total):
        check_against_truncate_paths(make, whole, want)
    # an env kind that never terminates (whole=None): its paths are the rounds of max_path_length lock steps, every env's
    # path of a round ends at the same lock step -- round by round, then env by env, NOT env 0's three paths first
    L, rounds = 5, 3
    dones3 = torch.zeros((L * rounds, N), dtype=torch.uint8)
    dones3[L - 1::L] = 1
    rewards3 = torch.as_tensor(rng.randn(L * rounds, N).astype(np.float32))
    make3 = lambda: Trajectories(z3(2, L * rounds), z3(1, L * rounds), z3(1, L * rounds), torch.zeros(1), rewards3,
                                 dones3.clone(), L)
    for want in (3, L * N, L * N + 1, 2 * L * N + L + 2, rounds * L * N):
        check_against_truncate_paths(make3, None, want)
    tr3 = check_against_truncate_paths(make3, None, 2 * L * N + L + 2)
    assert bool(tr3.valid[:2 * L].all()) and bool(tr3.valid[2 * L:, 0].all()) and int(tr3.valid[2 * L:, 1].sum()) == 2
    assert int(tr3.valid[2 * L:, 2:].sum()) == 0 and int(tr3.dones[2 * L + 1, 1]) == 1


def listed(tr):
    from rllab_amd.sampler.trajectories import PathList
    env, t0, t1 = (x.numpy() for x in PathList(tr).index())
    return sorted(zip(env.tolist(), t0.tolist(), (t1 - t0 + 1).tolist()))


@pytest.mark.parametrize("want,whole,steps,paths", [c for c in LOOP_CASES if not c[1]])
def test_keep_first_on_the_hand_recording_keeps_what_the_reference_keeps(want, whole, steps, paths):
    """The ``whole_paths=False`` rows of LOOP_CASES are the reference's output on ``recording()``; env-major ranking
    keeps [(0,0,2), (0,2,3), (1,0,1)] for (6, False), the reference [(0,0,2), (1,0,3), (0,2,1)]."""
    from rllab_amd.sampler.trajectories import Trajectories
    from rllab_amd.sampler.vectorized_sampler import VectorizedSampler
    d, r = recording()
    z3 = lambda k: torch.zeros((k, steps, 2))
    tr = Trajectories(z3(2), z3(1), z3(1), torch.zeros(1), torch.as_tensor(r[:steps], dtype=torch.float32),
                      torch.as_tensor(d[:steps]).clone(), 100)
    VectorizedSampler._keep_first(tr, want, tr.valid_mask(True))
    assert listed(tr) == sorted(paths)
    assert int(tr.valid.sum()) == want


class StubSampler(object):
    """``VectorizedSampler._meet_batch_size`` on the CPU: launches are served from ``rows(a, b) -> (dones, rewards)`` of
    lock steps a .. b - 1 (at most ``serve`` per launch), the path scan is the torch one of ``Trajectories``.  Records
    the length of every launch and of every scan."""

    def __init__(self, rows, n, batch_size, mpl, whole=True, serve=None):
        import types
        from rllab_amd.sampler.trajectories import Trajectories
        from rllab_amd.sampler.vectorized_sampler import VectorizedSampler
        algo = types.SimpleNamespace(policy=None, max_path_length=mpl, batch_size=batch_size, whole_paths=whole, env=None)
        self.s = s = VectorizedSampler(algo, n_envs=n)
        s.vec_env = types.SimpleNamespace(terminates=True, n=n)
        self.launches, self.scans, self.t = [], [], 0

        def chunk(policy, steps, first):
            a = 0 if first else self.t
            b = a + (steps if serve is None else min(steps, serve))
            d, r = rows(a, b)
            self.t = a + d.shape[0]
            self.launches.append(d.shape[0])
            z3 = lambda k: torch.zeros((k, d.shape[0], n))
            return Trajectories(z3(2), z3(1), z3(1), torch.zeros(1), torch.as_tensor(r, dtype=torch.float32),
                                torch.as_tensor(d).clone(), mpl)

        def path_index(traj):
            self.scans.append(traj.T)
            return traj.time_in_path().to(torch.int32), traj.valid_mask(True)
        s._rollout_chunk, s._path_index = chunk, path_index

    def run(self, first_steps):
        s = self.s
        return s._meet_batch_size(None, s._launch(None, first_steps, True))


@pytest.mark.parametrize("first_steps", [1, 2, 6])
@pytest.mark.parametrize("want,whole,steps,paths", LOOP_CASES)
def test_meet_batch_size_on_the_hand_recording_is_the_reference_loop(want, whole, steps, paths, first_steps):
    """The extension loop itself against the reference's recorded answers: wherever the launches' seams fall (a first
    launch of 1, 2 or all 6 lock steps, further launches of at most 2), the batch is cut at the reference's lock step
    and lists the reference's paths -- the running count and the running path lengths are carried over the seams."""
    d, r = recording()

    def rows(a, b):
        if a >= 6:
            raise RuntimeError("the sampler asks for lock step %d, the recording has 6" % a)
        return d[a:min(b, 6)], r[a:min(b, 6)]
    stub = StubSampler(rows, 2, want, 100, whole=whole, serve=2)
    tr = stub.run(first_steps)
    assert tr.T == steps
    if whole:
        tr.valid = tr.valid_mask(True)
    assert listed(tr) == sorted(paths)
    assert sum(stub.launches) >= steps and stub.scans[:len(stub.launches)] == stub.launches   # each launch scanned once, alone


def test_a_long_batch_on_one_env_is_bounded_by_progress_not_by_a_launch_count():
    """One env, paths of 5 lock steps, launches of at most 5: batch_size 2000 takes 400 launches.  The loop goes on
    while paths finish (the reference's just keeps looping), every launch is scanned on its own, and the batch is the
    400 whole paths."""
    def rows(a, b):
        t = np.arange(a, b)
        return (t % 5 == 4).astype(np.uint8).reshape(-1, 1), t.astype(np.float64).reshape(-1, 1)
    stub = StubSampler(rows, 1, 2000, 5, serve=5)
    tr = stub.run(5)
    assert tr.T == 2000 and len(stub.launches) == 400
    assert max(stub.scans) == 5 and len(stub.scans) == 400             # the work per launch does not grow
    # without the artificial limit on a launch: sized from the shortfall, NOT clamped to max_path_length when a round of
    # the envs cannot cover it -- a handful of launches instead of 400
    stub = StubSampler(rows, 1, 2000, 5)
    assert stub.run(5).T == 2000 and len(stub.launches) <= 3


def test_a_batch_that_cannot_finish_ends_with_a_clear_error():
    """No horizon and a ``done`` that never fires: no path ever finishes.  The loop gives up after MAX_STALLED_CHUNKS
    consecutive launches without a new finished sample -- a bound on progress -- and says what happened."""
    from rllab_amd.sampler.vectorized_sampler import VectorizedSampler
    rows = lambda a, b: (np.zeros((b - a, 3), np.uint8), np.zeros((b - a, 3)))
    stub = StubSampler(rows, 3, 100, 0)
    with pytest.raises(RuntimeError, match="no env has ended a path in the last .* done never fires"):
        stub.run(10)
    assert len(stub.launches) == VectorizedSampler.MAX_STALLED_CHUNKS
    # the same envs with ONE path ending every 40 lock steps: slow, but it is progress, and the batch completes
    rows = lambda a, b: ((np.arange(a, b) % 40 == 39).astype(np.uint8).reshape(-1, 1) * np.ones((1, 3), np.uint8),
                         np.zeros((b - a, 3)))
    stub = StubSampler(rows, 3, 1000, 0, serve=8)
    tr = stub.run(8)
    assert tr.T == 360 and len(stub.launches) == 45 > VectorizedSampler.MAX_STALLED_CHUNKS
