"""rl_ddpg_update (csrc/ddpg_kernels.hip) against the restatements of tests/ddpg_restatement.py.

Yardsticks: the five steps of an update as torch expressions with autograd, float64 and float32, on the CPU.  Rule (the
project's, tests/test_gpu_gru_bptt.py): per block, on the block's own norm, the kernel's error against float64 is at most
8 x the float32 restatement's, the yardstick floored at 2^-20.  What is compared is the MOVEMENT theta_after -
theta_before of every block of both nets and both targets -- the parameters themselves hardly move.  Adam divides the
gradient's scale away, so gradients are measured with SGD on both nets (movement = -lr x gradient) at rates that move a
block by 1e-3 .. 1e-1 of its norm (tests/ddpg_restatement.py::BIG_STEPS); Adam has its own tests.  Pools of 512 rows,
caller-supplied batch rows unless a test says otherwise.
"""
import numpy as np
import pytest
import torch

from tests import ddpg_restatement as R

pytestmark = pytest.mark.gpu


def _setup(cfg, st, pool, top=0, size=R.POOL_ROWS):
    """(FusedDDPGUpdate, DeviceReplayPool) on the device holding state ``st`` and pool ``pool`` (CPU tensors)."""
    from rllab_amd.algos.ddpg_update import FusedDDPGUpdate
    from rllab_amd.algos.replay_pool import DeviceReplayPool
    from rllab_amd.core.network import rectify, tanh
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab_amd.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    from rllab_amd.spaces import Box
    D, A = cfg["D"], cfg["A"]
    spec = EnvSpec(Box(-1e6 * np.ones(D), 1e6 * np.ones(D)), Box(-np.ones(A), np.ones(A)))
    f = {"rectify": rectify, "tanh": tanh}[cfg["hact"]]
    pol = DeterministicMLPPolicy(spec, hidden_sizes=cfg["hs"], hidden_nonlinearity=f,
                                 output_nonlinearity={"tanh": tanh, None: None}[cfg["oact"]])
    qf = ContinuousMLPQFunction(spec, hidden_sizes=cfg["hs"], hidden_nonlinearity=f)
    upd = FusedDDPGUpdate(pol, qf, cfg["B"])
    upd.load(st["pi"], st["q"], st["tpi"], st["tq"])
    dpool = DeviceReplayPool(pool["rew"].shape[0], D, A)
    for name in dpool.PLANES:
        getattr(dpool, name).copy_(pool[name])
    dpool.top, dpool.size = top, size
    return upd, dpool


def _kw(cfg, **over):
    kw = dict(discount=cfg["discount"], tau=cfg["tau"], qf_learning_rate=cfg["qf_lr"], policy_learning_rate=cfg["pi_lr"],
              qf_weight_decay=cfg["qf_wd"], policy_weight_decay=cfg["pi_wd"], qf_method=cfg["qf_method"],
              policy_method=cfg["pi_method"])
    kw.update(over)
    return kw


def _read(upd):
    pi, q = upd.unpack(0)
    tpi, tq = upd.unpack(1)
    return dict(pi=pi.double().cpu(), q=q.double().cpu(), tpi=tpi.double().cpu(), tq=tq.double().cpu())


def _run(cfg, st, pool, idx, **over):
    """K = len(idx) updates in one launch at rows ``idx``: (state read back, q_out, y_out, stats dict, updater)."""
    upd, dpool = _setup(cfg, st, pool)
    K = idx.shape[0]
    dev = upd.device
    q_out = torch.zeros((K, cfg["B"]), dtype=torch.float32, device=dev)
    y_out = torch.zeros_like(q_out)
    upd.update(dpool, K, indices=idx.to(dev).contiguous(), q_out=q_out, y_out=y_out, **_kw(cfg, **over))
    torch.cuda.synchronize()
    return _read(upd), q_out.double().cpu(), y_out.double().cpu(), upd.read_stats(reset=False), upd


def _scalar_within(name, got, ref64, ref32):
    got, ref64, ref32 = (torch.as_tensor(x, dtype=torch.float64).reshape(-1) for x in (got, ref64, ref32))
    R.within_blocks(name, got, ref64, ref32, [("all", 0, got.numel())])


_REF = {}


def _one_update_refs(kind, shape, batch):
    """float64 and float32 restatements of ONE update of a shared case at its batch ``batch``, computed once."""
    key = (kind, shape, batch)
    if key not in _REF:
        case = getattr(R, kind + "_case")(shape)
        cfg, st, pool, idx = case
        _REF[key] = (case, R.restated_update(cfg, st, pool, idx[batch], torch.float64),
                     R.restated_update(cfg, st, pool, idx[batch], torch.float32))
    return _REF[key]


@pytest.mark.parametrize("batch", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_one_sgd_update(shape, batch):
    """Movement of every block of theta_pi, theta_Q and both targets; q_out, y_out, qf_loss and surr on their own norms."""
    (cfg, st, pool, idx), (a64, o64), (a32, o32) = _one_update_refs("sgd", shape, batch)
    after, q_out, y_out, stats, upd = _run(cfg, st, pool, idx[batch:batch + 1])
    assert upd.step_counts() == (1, 1) and stats["updates"] == 1.0 and stats["samples"] == cfg["B"]
    R.within_blocks("movement %r" % (shape,), R.movement(st, after), R.movement(st, a64), R.movement(st, a32),
                    R.movement_blocks(cfg))
    _scalar_within("q_out", q_out[0], o64["q"], o32["q"])
    _scalar_within("y_out", y_out[0], o64["y"], o32["y"])
    _scalar_within("qf_loss", stats["qf_loss"], o64["qf_loss"], o32["qf_loss"])
    _scalar_within("surr", stats["policy_surr"], o64["surr"], o32["surr"])


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_weight_decay_scale(shape):
    """SGD with decay 0.1 on both nets: the decay term has the right factor on the weights and none on the biases (the
    restatement with decay on the biases misses the rule: tests/test_ddpg_host.py)."""
    (cfg, st, pool, idx), (a64, _), (a32, _) = _one_update_refs("decay", shape, 0)
    after = _run(cfg, st, pool, idx[0:1])[0]
    R.within_blocks("decay movement %r" % (shape,), R.movement(st, after), R.movement(st, a64), R.movement(st, a32),
                    R.movement_blocks(cfg))


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=str)
def test_order_q_step_then_policy_step(shape):
    """With a large Q rate the policy step's gradient depends on which Q parameters it sees: the kernel matches the
    restatement in the reference's order and misses the one with the two steps swapped."""
    (cfg, st, pool, idx), (a64, _), (a32, _) = _one_update_refs("order", shape, 0)
    after = _run(cfg, st, pool, idx[0:1])[0]
    got, ref64, ref32 = R.movement(st, after), R.movement(st, a64), R.movement(st, a32)
    R.within_blocks("order %r" % (shape,), got, ref64, ref32, R.movement_blocks(cfg))
    swapped = R.movement(st, R.restated_update(cfg, st, pool, idx[0], torch.float64, swap_order=True)[0])
    e32 = R.rel_errors(ref32, ref64, R.movement_blocks(cfg))
    e_sw = R.rel_errors(got, swapped, R.movement_blocks(cfg))
    for name in ("pi.W0", "pi.W1", "pi.W2", "pi.b2"):
        assert e_sw[name] > R.ALLOW * max(e32[name], R.FLOOR), (name, e_sw[name], e32[name])


def test_padded_entries_stay_zero():
    """20 Adam updates with weight decay at hidden (20, 7): every entry of theta, targets, m and v outside the real
    parameters is an exact zero (B = 33: the gradient scratch of a second chunk is in use too)."""
    cfg, st, pool, _ = R.adam_case(R.SHAPES[2])
    idx = R.make_indices(cfg, 20, seed=5)
    upd = _run(cfg, st, pool, idx)[4]
    real = torch.zeros(upd.P, dtype=torch.bool, device=upd.device)
    real[upd.idx_policy] = True
    real[upd.idx_qf] = True
    assert int((~real).sum()) > 2000
    for k, name in enumerate(("theta", "targets", "m", "v")):
        plane = upd.plane(k)
        assert bool(torch.all(plane[~real] == 0)), name
        assert bool(torch.any(plane[real] != 0)), name
    assert upd.step_counts() == (20, 20)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[1], R.SHAPES[2]], ids=str)
def test_k_updates_in_one_launch_equal_k_launches(shape):
    """K = 50 in one launch == 50 launches of K = 1, and K = 3 == 1 + 2 (the Adam step count is carried in the state):
    the whole state buffer, bit for bit.  Adam with decay on both nets."""
    cfg, st, pool, _ = R.adam_case(shape)
    idx = R.make_indices(cfg, 50, seed=6)
    one = _run(cfg, st, pool, idx)[4]
    upd, dpool = _setup(cfg, st, pool)
    dev_idx = idx.to(upd.device)
    for k in range(50):
        upd.update(dpool, 1, indices=dev_idx[k:k + 1].contiguous(), **_kw(cfg))
    torch.cuda.synchronize()
    assert upd.step_counts() == (50, 50) == one.step_counts()
    n = 4 * upd.P        # theta, targets, m, v (the scratch plane behind them is scratch)
    assert torch.equal(one.state[:n].view(torch.int32), upd.state[:n].view(torch.int32))
    assert torch.equal(one.stats, upd.stats)
    three = _run(cfg, st, pool, idx[:3])[4]
    upd, dpool = _setup(cfg, st, pool)
    upd.update(dpool, 1, indices=dev_idx[0:1].contiguous(), **_kw(cfg))
    upd.update(dpool, 2, indices=dev_idx[1:3].contiguous(), **_kw(cfg))
    torch.cuda.synchronize()
    assert upd.step_counts() == (3, 3)
    assert torch.equal(three.state[:n].view(torch.int32), upd.state[:n].view(torch.int32))


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_fifty_adam_updates(shape):
    """50 Adam updates (decay on) against the float64 restatement within the rule; a second run gives the same bits."""
    cfg, st, pool, _ = R.adam_case(shape)
    idx = R.make_indices(cfg, 50, seed=7)
    a64 = R.run_updates(cfg, st, pool, idx, torch.float64)[0]
    a32 = R.run_updates(cfg, st, pool, idx, torch.float32)[0]
    after, q1, y1, _, upd1 = _run(cfg, st, pool, idx)
    R.within_blocks("50 Adam updates %r" % (shape,), R.movement(st, after), R.movement(st, a64), R.movement(st, a32),
                    R.movement_blocks(cfg))
    _, q2, y2, _, upd2 = _run(cfg, st, pool, idx)
    n = 4 * upd1.P
    assert torch.equal(upd1.state[:n].view(torch.int32), upd2.state[:n].view(torch.int32))
    assert torch.equal(q1, q2) and torch.equal(y1, y2)


def test_terminal_rows_give_y_equal_reward():
    cfg, st, pool, idx = R.sgd_case(R.SHAPES[0])
    pool = dict(pool, term=torch.ones_like(pool["term"]))
    _, _, y_out, _, _ = _run(cfg, st, pool, idx[0:1])
    want = pool["rew"][idx[0].long()]
    assert torch.equal(y_out[0].float().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=str)
def test_soft_target_extremes(shape):
    """tau = 1: the targets ARE the parameters just written; tau = 0: the targets are untouched.  Bit for bit."""
    cfg, st, pool, idx = R.sgd_case(shape)
    upd = _run(cfg, st, pool, idx[0:1], tau=1.0)[4]
    assert torch.equal(upd.plane(0).view(torch.int32), upd.plane(1).view(torch.int32))
    assert not torch.equal(upd.unpack(0)[0].cpu(), st["pi"].float())       # (the parameters did move)
    upd = _run(cfg, st, pool, idx[0:1], tau=0.0)[4]
    tpi, tq = upd.unpack(1)
    assert torch.equal(tpi.cpu().view(torch.int32), st["tpi"].float().view(torch.int32))
    assert torch.equal(tq.cpu().view(torch.int32), st["tq"].float().view(torch.int32))


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=str)
def test_decay_alone_moves_weights_and_not_biases(shape):
    """A zero learning signal: every batch row is terminal with reward = Q(s, a) (read from a first launch at rate 0), so
    y = q bit for bit and the Q loss has gradient zero; the action rows of Q's W1 are zero, so the policy's surrogate
    has gradient zero.  SGD at rate 0.5 with decay 0.1 then moves every weight by -0.05 w -- to 3 roundings of
    2^-24 |w| against a movement of 0.05 |w|, i.e. 3.6e-6 relative; 1e-5 is asserted -- and leaves every bias unchanged,
    bit for bit."""
    cfg, st, pool, idx = R.sgd_case(shape)
    D, A, hs = cfg["D"], cfg["A"], cfg["hs"]
    st = dict(st)
    q = st["q"].clone()
    (_, b, e) = R.blocks(D, A, hs, A, 1)[2]
    q[b:e].reshape(hs[0] + A, hs[1])[hs[0]:] = 0.0
    st["q"] = q
    pool = dict(pool, term=torch.ones_like(pool["term"]))
    zero = dict(qf_learning_rate=0.0, policy_learning_rate=0.0, tau=0.0)
    q_out = _run(cfg, st, pool, idx[0:1], **zero)[1]
    rew = pool["rew"].clone()
    rew[idx[0].long()] = q_out[0].float()
    pool = dict(pool, rew=rew)
    after, q2, y2, _, _ = _run(cfg, st, pool, idx[0:1], qf_learning_rate=0.5, policy_learning_rate=0.5,
                               qf_weight_decay=0.1, policy_weight_decay=0.1, tau=0.0)
    assert torch.equal(q2, y2)
    for key, merge, out in (("pi", 0, A), ("q", A, 1)):
        for name, b, e in R.blocks(D, A, hs, merge, out):
            w0, w1 = st[key][b:e], after[key][b:e]
            if name.startswith("b"):
                assert torch.equal(w0.float().view(torch.int32), w1.float().view(torch.int32)), (key, name)
            else:
                err = float((w1 - w0 + 0.05 * w0).norm()) / float((0.05 * w0).norm())
                print(key, name, err)
                assert err <= 1e-5, (key, name, err)


@pytest.mark.parametrize("pool_kind", ["wrapped", "half skipped"])
def test_in_kernel_draws(pool_kind):
    """indices_out of a launch that draws its own batches == the numpy restatement of the rule, exactly; a launch fed
    those rows through args.indices gives the same bits."""
    cfg, st, pool, _ = R.adam_case(R.SHAPES[0])
    if pool_kind == "wrapped":
        top, size, skip = 40, 300, torch.zeros(R.POOL_ROWS)
    else:
        top, size = 0, R.POOL_ROWS
        skip = torch.as_tensor((np.random.RandomState(9).rand(R.POOL_ROWS) < 0.5).astype(np.float32))
    pool = dict(pool, skip=skip)
    K, B, seed, base = 6, cfg["B"], 0x1234567890ABCDEF, (1 << 32) - 2          # the counter crosses 2^32
    upd, dpool = _setup(cfg, st, pool, top=top, size=size)
    rows = torch.zeros((K, B), dtype=torch.int32, device=upd.device)
    upd.update(dpool, K, seed=seed, update_base=base, indices_out=rows, **_kw(cfg))
    torch.cuda.synchronize()
    want = np.stack([R.draw_rows(seed, base + u, B, size, top, R.POOL_ROWS, skip.numpy()) for u in range(K)])
    assert np.array_equal(rows.cpu().numpy(), want)
    assert not skip[rows.cpu().long()].any()
    fed, dpool2 = _setup(cfg, st, pool, top=top, size=size)
    fed.update(dpool2, K, indices=rows, **_kw(cfg))
    torch.cuda.synchronize()
    n = 4 * upd.P
    assert torch.equal(upd.state[:n].view(torch.int32), fed.state[:n].view(torch.int32))
    assert torch.equal(upd.stats, fed.stats)


def test_statistics_block():
    """The float64 sums on the device == the sums over q_out / y_out formed here in float64, to 1e-12 relative."""
    cfg, st, pool, _ = R.adam_case(R.SHAPES[2])
    idx = R.make_indices(cfg, 7, seed=8)
    _, q, y, stats, _ = _run(cfg, st, pool, idx)
    want = dict(qf_loss=float(((y - q) ** 2).mean(dim=1).sum()), updates=7.0, q=float(q.sum()), abs_q=float(q.abs().sum()),
                y=float(y.sum()), abs_y=float(y.abs().sum()), abs_q_y_diff=float((q - y).abs().sum()),
                samples=7.0 * cfg["B"])
    for k, v in want.items():
        assert abs(stats[k] - v) <= 1e-12 * max(abs(v), 1e-300), (k, stats[k], v)
    assert np.isfinite(stats["policy_surr"]) and stats["policy_surr"] != 0.0


def test_guard_rails():
    """size <= batch is refused before anything is launched; rows out of range are clamped into the pool."""
    cfg, st, pool, idx = R.sgd_case(R.SHAPES[0])
    upd, dpool = _setup(cfg, st, pool, top=32, size=32)
    with pytest.raises(RuntimeError, match="must exceed the batch"):
        upd.update(dpool, 1, indices=idx[0:1].to(upd.device), **_kw(cfg))
    upd, dpool = _setup(cfg, st, pool)
    wild = idx[0:1].clone()
    wild[0, 0], wild[0, 1] = -5, 10 ** 6
    rows = torch.zeros((1, cfg["B"]), dtype=torch.int32, device=upd.device)
    upd.update(dpool, 1, indices=wild.to(upd.device), indices_out=rows, **_kw(cfg))
    torch.cuda.synchronize()
    got = rows.cpu()[0]
    assert int(got[0]) == 0 and int(got[1]) == R.POOL_ROWS - 1 and torch.equal(got[2:], idx[0, 2:])
