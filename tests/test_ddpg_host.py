"""DDPG without a device: the restatements the GPU tests measure against (tests/ddpg_restatement.py) agree with each
other and can see the mistakes they are there to catch; the batch-index rule; the exploration strategies, the policy /
Q-function objects, the replay pool's bookkeeping and the argument checks of rl_ddpg_update.

Power checks: a float64 restatement with ONE mistake built in (policy step before the Q step, loss summed instead of
averaged, decay on the biases, terminal mask dropped) must miss the accuracy rule against the right one on the inputs
the GPU tests use -- otherwise a kernel with that mistake would pass them.
"""
import ctypes
import pickle

import numpy as np
import pytest
import torch

from tests import ddpg_restatement as R


def _spec(D, A):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Box
    return EnvSpec(Box(-1e6 * np.ones(D), 1e6 * np.ones(D)), Box(-np.ones(A), np.ones(A)))


# ---- the restatements -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_float32_restatement_agrees_with_float64(shape):
    """One SGD update in float32 against float64, relative, on every block's own norm.  q, y, the loss and the
    surrogate: within ALLOW x FLOOR -- float32 carries 2^-24 per operation and the sums here are at most 128 x 72 terms
    long.  A block's movement: within that plus 4 x 2^-24 |theta| / |movement|, because the float32 parameters
    themselves are rounded to 2^-24 |theta| when they are stored (at most three roundings of that size on the way: two
    products, one sum)."""
    cfg, st, pool, idx = R.sgd_case(shape)
    a64, o64 = R.restated_update(cfg, st, pool, idx[0], torch.float64)
    a32, o32 = R.restated_update(cfg, st, pool, idx[0], torch.float32)
    mv64, bl = R.movement(st, a64), R.movement_blocks(cfg)
    errs = R.rel_errors(R.movement(st, a32), mv64, bl)
    theta = torch.cat([st[k] for k in ("pi", "q", "tpi", "tq")])
    bound = {n: R.ALLOW * R.FLOOR + 4 * 2.0 ** -24 * float(theta[b:e].norm()) / float(mv64[b:e].norm()) for n, b, e in bl}
    for k in ("q", "y", "qf_loss", "surr"):
        errs[k] = float((o32[k] - o64[k]).norm()) / float(o64[k].norm())
        bound[k] = R.ALLOW * R.FLOOR
    print({k: "%.2e of %.2e" % (errs[k], bound[k]) for k in errs})
    bad = {k: v for k, v in errs.items() if not v <= bound[k]}
    assert not bad, bad


def _missed_blocks(cfg, st, wrong, right64, right32):
    got, ref64, ref32 = R.movement(st, wrong), R.movement(st, right64), R.movement(st, right32)
    missed = []
    for name, b, e in R.movement_blocks(cfg):
        n64 = float(ref64[b:e].norm())
        e_w = float((got[b:e] - ref64[b:e]).norm()) / n64
        e_32 = float((ref32[b:e] - ref64[b:e]).norm()) / n64
        if e_w > R.ALLOW * max(e_32, R.FLOOR):
            missed.append((name, e_w / max(e_32, R.FLOOR)))
    return missed


def _power(case, must_miss, **variant):
    cfg, st, pool, idx = case
    right64, _ = R.restated_update(cfg, st, pool, idx[0], torch.float64)
    right32, _ = R.restated_update(cfg, st, pool, idx[0], torch.float32)
    wrong, _ = R.restated_update(cfg, st, pool, idx[0], torch.float64, **variant)
    missed = dict(_missed_blocks(cfg, st, wrong, right64, right32))
    print(variant, missed)
    for name in must_miss:
        assert name in missed, (variant, name, missed)


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=str)
def test_power_order_of_q_and_policy_step(shape):
    """The policy step at the OLD Q parameters moves every policy block (and its target) visibly differently."""
    _power(R.order_case(shape), ["pi.W0", "pi.b0", "pi.W1", "pi.b1", "pi.W2", "pi.b2", "targ_pi.W0", "targ_pi.W2"],
           swap_order=True)


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[4] > 1], ids=str)
def test_power_mean_over_the_batch(shape):
    _power(R.sgd_case(shape), ["pi.W0", "pi.b2", "q.W0", "q.W1", "q.b2", "targ_q.W1"], no_mean=True)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_power_decay_on_weights_only(shape):
    _power(R.decay_case(shape), ["pi.b0", "pi.b1", "pi.b2", "q.b0", "q.b1", "q.b2"], decay_biases=True)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_power_terminal_mask(shape):
    cfg, st, pool, idx = R.sgd_case(shape)
    assert float(pool["term"][idx[0].long()].sum()) >= 1          # the batch holds a terminal row
    _power((cfg, st, pool, idx), ["q.W0", "q.W1", "q.W2", "q.b2"], drop_term=True)


# ---- the batch-index rule -------------------------------------------------------------------------------------------
def test_draw_rows_range_wrap_and_skip():
    cap, B = 512, 128
    none = np.zeros(cap)
    rows = R.draw_rows(7, 0, B, 100, 100, cap, none)              # a pool that has not wrapped: rows 0 .. 99
    assert rows.min() >= 0 and rows.max() < 100
    rows = np.concatenate([R.draw_rows(7, c, B, 300, 40, cap, none) for c in range(8)])    # top < size: a ring wrap
    live = set(range(0, 40)) | set(range(cap - 260, cap))
    assert set(rows.tolist()) <= live
    assert (rows < 40).any() and (rows >= cap - 260).any()
    skip = (np.random.RandomState(0).rand(cap) < 0.5).astype(np.float32)
    rows = np.concatenate([R.draw_rows(11, c, B, cap, 0, cap, skip) for c in range(16)])
    assert not skip[rows].any()
    # two updates, two slots: different words
    assert not np.array_equal(R.draw_rows(7, 0, B, cap, 0, cap, none), R.draw_rows(7, 1, B, cap, 0, cap, none))
    assert not np.array_equal(R.draw_rows(7, 0, B, cap, 0, cap, none), R.draw_rows(8, 0, B, cap, 0, cap, none))


def test_draw_rows_terminates_with_one_kept_row_and_with_none():
    cap, size, top = 64, 50, 20
    skip = np.ones(cap, dtype=np.float32)
    kept = (top - size + 17) % cap
    skip[kept] = 0
    assert R.draw_rows(3, 5, 32, size, top, cap, skip).tolist() == [kept] * 32
    skip[kept] = 1                                                  # nothing kept: still ends, inside the pool
    rows = R.draw_rows(3, 5, 32, size, top, cap, skip)
    live = {(top - size + i) % cap for i in range(size)}
    assert set(rows.tolist()) <= live


def test_draw_rows_are_uniform():
    """65 536 draws over 64 rows: Pearson's chi-square (63 degrees of freedom) below its 99.9 % quantile, 103.44."""
    rows = np.concatenate([R.draw_rows(20161021, c, 128, 64, 0, 64, np.zeros(64)) for c in range(512)])
    counts = np.bincount(rows, minlength=64).astype(np.float64)
    chi2 = float(((counts - 1024.0) ** 2 / 1024.0).sum())
    print("chi-square", chi2)
    assert chi2 < 103.44


# ---- exploration strategies -----------------------------------------------------------------------------------------
class _FixedPolicy(object):
    def __init__(self, actions):
        self.actions = actions

    def get_actions(self, observations):
        return self.actions, dict()

    def get_action(self, observation):
        return self.actions[0].numpy().astype(np.float64), dict()


def test_ou_strategy_formula_reset_and_clipping():
    from rllab_amd.exploration_strategies.ou_strategy import OUStrategy
    es = OUStrategy(_spec(3, 2), mu=0.1, theta=0.2, sigma=0.4)
    rng = np.random.RandomState(0)
    pol = _FixedPolicy(torch.as_tensor(rng.uniform(-0.5, 0.5, (5, 2)).astype(np.float32)))
    x = np.full((5, 2), 0.1)
    for t in range(4):
        z = rng.randn(5, 2).astype(np.float32)
        got = es.get_actions(t, torch.zeros(5, 3), pol, normals=torch.as_tensor(z))
        x = x + 0.2 * (0.1 - x) + 0.4 * z.astype(np.float64)
        want = np.clip(pol.actions.numpy().astype(np.float64) + x, -1.0, 1.0)
        assert np.allclose(got.numpy(), want, atol=1e-6)
        if t == 1:                                                  # envs 1 and 3 end a path: their rows start over
            es.reset(mask=torch.tensor([False, True, False, True, False]))
            x[[1, 3]] = 0.1
    assert np.allclose(es.states.numpy(), x, atol=1e-6)
    big = _FixedPolicy(torch.full((5, 2), 3.0))
    assert float(es.get_actions(0, torch.zeros(5, 3), big, normals=torch.zeros(5, 2)).max()) == 1.0
    es.reset()
    assert np.allclose(es.states.numpy(), 0.1) and np.allclose(es.state, 0.1)
    # the single-env face and a pickle round trip of its state
    np.random.seed(0)
    a = es.get_action(0, np.zeros(3), pol)
    assert a.shape == (2,) and np.all(np.abs(a) <= 1.0)
    twin = pickle.loads(pickle.dumps(es))
    assert np.array_equal(twin.state, es.state) and twin.theta == 0.2


def test_gaussian_strategy_sigma_schedule():
    from rllab_amd.exploration_strategies.gaussian_strategy import GaussianStrategy
    es = GaussianStrategy(_spec(3, 2), max_sigma=1.0, min_sigma=0.1, decay_period=1000)
    assert es.sigma(0) == 1.0 and abs(es.sigma(500) - 0.55) < 1e-12 and abs(es.sigma(1000) - 0.1) < 1e-12
    assert abs(es.sigma(5000) - 0.1) < 1e-12
    pol = _FixedPolicy(torch.zeros(4, 2))
    z = torch.as_tensor(np.random.RandomState(1).randn(4, 2).astype(np.float32))
    got = es.get_actions(500, torch.zeros(4, 3), pol, normals=z)
    assert np.allclose(got.numpy(), np.clip(0.55 * z.numpy(), -1, 1), atol=1e-6)


# ---- policy and Q-function objects ----------------------------------------------------------------------------------
def test_policy_and_qf_initialisation_order_and_pickle():
    from rllab_amd.core.network import rectify, tanh
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab_amd.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    spec = _spec(13, 2)
    np.random.seed(0)
    pol = DeterministicMLPPolicy(spec, hidden_sizes=(20, 7))
    qf = ContinuousMLPQFunction(spec, hidden_sizes=(20, 7))
    assert pol.hidden_nonlinearity is rectify and pol.output_nonlinearity is tanh and qf.output_nonlinearity is None
    assert [p.shape for p in pol.get_params()] == [(13, 20), (20,), (20, 7), (7,), (7, 2), (2,)]
    assert [p.shape for p in qf.get_params()] == [(13, 20), (20,), (22, 7), (7,), (7, 1), (1,)]
    assert qf.action_merge_layer == 1
    assert [p.shape for p in pol.get_params(regularizable=True)] == [(13, 20), (20, 7), (7, 2)]
    assert [p.shape for p in qf.get_params(regularizable=True)] == [(13, 20), (22, 7), (7, 1)]
    for obj, fan in ((pol, (13, 20)), (qf, (13, 22))):
        W0, b0, W1, b1, W2, b2 = [p.get_value() for p in obj.get_params()]
        for W, f in ((W0, fan[0]), (W1, fan[1])):
            bound = np.sqrt(6.0 / f)                               # He-uniform
            assert np.abs(W).max() <= bound and np.abs(W).max() > 0.8 * bound
        assert not b0.any() and not b1.any()
        assert np.abs(W2).max() <= 3e-3 and np.abs(b2).max() <= 3e-3 and W2.any() and b2.any()
    # flat order = the blocks the restatement splits
    flat = torch.as_tensor(pol.get_param_values())
    cfg = R.make_cfg(13, 2, (20, 7), "rectify", 4)
    obs = torch.as_tensor(np.random.RandomState(1).randn(4, 13))
    assert np.allclose(pol.get_actions(obs.float())[0].numpy(), R.pi_forward(flat, obs, cfg).numpy(), atol=1e-6)
    act = torch.as_tensor(np.random.RandomState(2).uniform(-1, 1, (4, 2)))
    assert np.allclose(qf.get_qval(obs.numpy(), act.numpy()),
                       R.q_forward(torch.as_tensor(qf.get_param_values()), obs, act, cfg).numpy(), atol=1e-6)
    a, info = pol.get_action(obs[0].numpy())
    assert a.shape == (2,) and info == dict()
    for obj in (pol, qf):
        twin = pickle.loads(pickle.dumps(obj))
        assert np.array_equal(twin.get_param_values(), obj.get_param_values())
        obj.set_param_values(obj.get_param_values() + 1.0)
        assert not np.array_equal(twin.get_param_values(), obj.get_param_values())
    with pytest.raises(NotImplementedError, match="batch normalisation"):
        DeterministicMLPPolicy(spec, bn=True)
    with pytest.raises(NotImplementedError, match="batch normalisation"):
        ContinuousMLPQFunction(spec, bn=True)


def test_state_layout_round_trip_and_refusals():
    """The padded state layout takes the objects' vectors and hands them back; what the kernel does not run is named."""
    from rllab_amd.algos.ddpg_update import ddpg_why_unsupported, net_index
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab_amd.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    from rllab_amd import _lib
    for D, A, hs, _, _ in R.SHAPES:
        ip, iq, P = net_index(D, A, hs)
        assert len(np.unique(np.concatenate([ip, iq]))) == len(ip) + len(iq) and iq.max() < P
        assert _lib.lib.rl_ddpg_state_bytes(D, A, hs[0], hs[1]) >= (5 * P + 2) * 4
    # Q's W1: hidden rows, then the action rows behind the PADDED hidden rows
    ip, iq, P = net_index(13, 2, (20, 7))
    base_q = 13 * 32 + 32 + 32 * 32 + 32 + 32 * 2 + 2
    w1 = base_q + 13 * 32 + 32
    assert iq[13 * 20 + 20] == w1 and iq[13 * 20 + 20 + 20 * 7] == w1 + 32 * 32
    spec = _spec(4, 1)
    ok = lambda **kw: DeterministicMLPPolicy(spec, **kw)
    qf = ContinuousMLPQFunction(spec)
    assert ddpg_why_unsupported(ok(), qf) is None
    assert "at most 64 units" in ddpg_why_unsupported(ok(hidden_sizes=(128, 128)),
                                                      ContinuousMLPQFunction(spec, hidden_sizes=(128, 128)))
    assert "two hidden layers" in ddpg_why_unsupported(ok(hidden_sizes=(32, 32, 32)), qf)
    assert "differ" in ddpg_why_unsupported(ok(hidden_sizes=(32, 16)), qf)
    assert "1 .. 128" in ddpg_why_unsupported(ok(), qf, batch_size=129)
    assert "hidden layer 1" in ddpg_why_unsupported(ok(), ContinuousMLPQFunction(spec, action_merge_layer=0))
    assert _lib.lib.rl_ddpg_state_bytes(33, 1, 32, 32) == 0 and _lib.lib.rl_ddpg_state_bytes(4, 9, 32, 32) == 0
    assert _lib.lib.rl_ddpg_state_bytes(4, 1, 65, 32) == 0 and _lib.lib.rl_ddpg_state_bytes(4, 1, 32, 0) == 0


# ---- the replay pool ------------------------------------------------------------------------------------------------
def test_replay_pool_bookkeeping():
    from rllab_amd.algos.replay_pool import DeviceReplayPool
    pool = DeviceReplayPool(10, 3, 2, device="cpu")
    assert (pool.top, pool.size) == (0, 0)
    step = 0
    for n_rows in (4, 4, 4, 3):                                     # 15 rows through a ring of 10: wraps mid-write
        ids = torch.arange(step, step + n_rows, dtype=torch.float32)
        pool.add(ids[:, None].expand(-1, 3), -ids[:, None].expand(-1, 2), ids * 10, (ids % 2 == 0), ids[:, None] + 0.5 +
                 torch.zeros(n_rows, 3), (ids % 3 == 0))
        step += n_rows
    assert (pool.top, pool.size) == (5, 10)
    want = np.array([10, 11, 12, 13, 14, 5, 6, 7, 8, 9], dtype=np.float32)      # row r holds transition want[r]
    assert np.array_equal(pool.obs[:, 0].numpy(), want) and np.array_equal(pool.act[:, 1].numpy(), -want)
    assert np.array_equal(pool.rew.numpy(), want * 10) and np.array_equal(pool.next_obs[:, 2].numpy(), want + 0.5)
    assert np.array_equal(pool.term.numpy(), (want % 2 == 0).astype(np.float32))
    assert np.array_equal(pool.skip.numpy(), (want % 3 == 0).astype(np.float32))
    assert pool.logical_rows().tolist() == [5, 6, 7, 8, 9, 0, 1, 2, 3, 4]      # oldest first
    pool.add(torch.zeros(1, 3), torch.zeros(1, 2), torch.zeros(1), torch.zeros(1), torch.zeros(1, 3))
    assert (pool.top, pool.size) == (6, 10) and float(pool.skip[5]) == 0.0
    with pytest.raises(ValueError):
        pool.add(torch.zeros(11, 3), torch.zeros(11, 2), torch.zeros(11), torch.zeros(11), torch.zeros(11, 3))


# ---- argument checks of the entry point -----------------------------------------------------------------------------
def test_rl_ddpg_update_argument_errors_without_a_device():
    from rllab_amd import _lib
    lib = _lib.lib
    assert lib.rl_ddpg_update(None, None) == -1 and b"rl_ddpg_update" in lib.rl_last_error()

    def args(**kw):
        a = _lib.DdpgArgs(obs_dim=4, act_dim=1, hidden0=32, hidden1=32, hidden_activation=_lib.ACT_RECTIFY,
                          output_activation=_lib.ACT_TANH, batch=32, n_updates=1, capacity=512, size=100, top=100,
                          qf_method=0, policy_method=0, discount=0.99, tau=0.001, qf_learning_rate=1e-3,
                          policy_learning_rate=1e-4)
        for name in ("state", "obs", "act", "rew", "term", "next_obs", "skip"):
            setattr(a, name, 64)                                    # never dereferenced: every case below is refused
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(obs_dim=0), dict(obs_dim=33), dict(act_dim=0), dict(act_dim=9), dict(hidden0=0), dict(hidden0=65),
           dict(hidden1=0), dict(hidden1=128), dict(hidden_activation=_lib.ACT_IDENTITY), dict(hidden_activation=7),
           dict(output_activation=_lib.ACT_RECTIFY), dict(output_activation=-1), dict(batch=0), dict(batch=129),
           dict(n_updates=0), dict(n_updates=16385), dict(capacity=0), dict(size=0), dict(size=513), dict(top=-1),
           dict(top=512), dict(size=32), dict(size=20), dict(qf_method=2), dict(policy_method=-1),
           dict(tau=-0.1), dict(tau=1.5), dict(tau=float("nan")), dict(discount=float("inf")),
           dict(qf_learning_rate=float("nan")), dict(policy_weight_decay=float("inf")),
           dict(state=None), dict(obs=None), dict(act=None), dict(rew=None), dict(term=None), dict(next_obs=None),
           dict(skip=None)]
    for kw in bad:
        rc = lib.rl_ddpg_update(ctypes.byref(args(**kw)), None)
        msg = lib.rl_last_error()
        assert rc in (-1, -2) and msg.startswith(b"rl_ddpg_update"), (kw, rc, msg)
    rc = lib.rl_ddpg_update(ctypes.byref(args(hidden0=65)), None)
    assert rc == -2 and b"at most 64 units" in lib.rl_last_error()
    rc = lib.rl_ddpg_update(ctypes.byref(args(size=32)), None)
    assert rc == -1 and b"must exceed the batch" in lib.rl_last_error()


def test_alias_paths_import():
    import rllab.algos.ddpg
    import rllab.algos.replay_pool
    import rllab.exploration_strategies.gaussian_strategy
    import rllab.exploration_strategies.ou_strategy
    import rllab.policies.deterministic_mlp_policy
    import rllab.q_functions.continuous_mlp_q_function
    import rllab_amd.algos.ddpg
    assert rllab.algos.ddpg.DDPG is rllab_amd.algos.ddpg.DDPG
    assert rllab.q_functions.continuous_mlp_q_function.ContinuousMLPQFunction.__module__.startswith("rllab_amd")
