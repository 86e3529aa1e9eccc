"""Discrete actions on the GPU: the fused GridWorld rollout (rl_rollout_gridworld), the categorical head kernels
(rl_categorical_head / rl_categorical_fisher, csrc/categorical_kernels.hip) under the networks-on-planes kernels, and the
reference's test matrix -- GridWorldEnv with a CategoricalMLPPolicy (tests/test_algos.py:76-94 of rllab).

The rollout is replayed through the Python GridWorldEnv (integers: equality).  The update kernels are compared with
float64 autograd of the ``Categorical`` torch twins at the bars of tests/test_gpu_update_parity.py and
tests/test_gpu_wide_nets.py: loss, KL and vpg 2e-5 relative, gradients 2e-5 max|g|, Fisher-vector product 5e-5 max|Hv|.
Every parity case first asserts that the smallest probability in its batch is at least 1e-3: the reference's
TINY = 1e-8 then enters every quantity at O(1e-8 / p) <= 1e-5 RELATIVE to terms the kernels and the float64 twins both
carry (both keep TINY where the reference has it), far below the bars."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETWORKS = [(16, 4, (32, 32)), (16, 4, (20,)), (29, 4, (100, 50, 25))]
BATCHES = [1, 63, 1000, 70001]


# -- helpers ----------------------------------------------------------------------------------------------------------
def _policy(do, da, hidden, seed=0):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
    from rllab_amd.spaces import Discrete
    np.random.seed(seed)
    pol = CategoricalMLPPolicy(EnvSpec(Discrete(do), Discrete(da)), hidden_sizes=hidden)
    theta = pol.get_param_values()
    theta += 0.1 * np.random.randn(theta.size)
    pol.set_param_values(theta)
    return pol


def _grid_policy(desc, hidden=(32, 32), seed=0):
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    env = GridWorldEnv(desc)
    pol = _policy(env.observation_space.n, 4, hidden, seed)
    return env, pol


def _inputs(pol, B, seed=1, ragged=True, old_equals_new=False):
    """The batch of tests/test_gpu_update_parity.py::_inputs for a categorical policy: normal observation planes, old
    probabilities = the current ones (or the current logits moved by 0.05 N(0, 1)), actions drawn from the old
    distribution, normal advantages, a tenth of the weights zero."""
    rng = np.random.RandomState(seed)
    dev = pol.flat_params.device
    do, da = pol.obs_dim, pol.action_dim
    obs = torch.as_tensor(rng.randn(do, B).astype(np.float32), device=dev)
    with torch.no_grad():
        logits = pol.logit_planes(obs.double(), pol.flat_params.double())
        if not old_equals_new:
            logits = logits + 0.05 * torch.as_tensor(rng.randn(da, B), device=dev)
        old_prob = torch.softmax(logits, dim=0).float()
    cs = np.cumsum(old_prob.cpu().numpy().astype(np.float64), axis=0)
    idx = np.minimum((cs < rng.rand(B)[None, :]).sum(axis=0), da - 1)
    act = torch.as_tensor(np.eye(da, dtype=np.float32)[idx].T.copy(), device=dev)
    adv = torch.as_tensor(rng.randn(B).astype(np.float32), device=dev)
    w = torch.ones(B, dtype=torch.float32, device=dev)
    if ragged:
        w[torch.as_tensor(rng.rand(B) < 0.1, device=dev)] = 0.0
        w[0] = 1.0          # never an all-masked batch (1 / count would be inf)
    inv = 1.0 / w.double().sum()
    return (obs, act, adv, old_prob, w, inv)


def _closures(pol):
    dist = pol.distribution

    def new(flat, obs):
        return pol.dist_info_planes(obs.double(), flat.double())

    def surr(flat, obs, act, adv, op, w, inv):
        lr = dist.likelihood_ratio_sym(act.double(), dict(prob=op.double()), new(flat, obs), axis=0)
        return -(lr * adv.double() * w.double()).sum() * inv

    def kl(flat, obs, act, adv, op, w, inv):
        return (dist.kl_sym(dict(prob=op.double()), new(flat, obs), axis=0) * w.double()).sum() * inv

    def vpg(flat, obs, act, adv, op, w, inv):
        return -(dist.log_likelihood_sym(act.double(), new(flat, obs), axis=0) * adv.double() * w.double()).sum() * inv
    return surr, kl, vpg


def _min_prob(pol, inp):
    with torch.no_grad():
        now = pol.dist_info_planes(inp[0].double(), pol.flat_params.double())["prob"]
    return min(float(now.min()), float(inp[3].min()))


# -- the rollout against the host env ---------------------------------------------------------------------------------
def _replay(env, traj_chunks, n, max_path_length):
    """Every env's recorded actions through the Python GridWorldEnv with the executor's reset rule; asserts observations,
    rewards and dones of all chunks (consecutive launches of the same envs) and returns the final (state, ts) lists."""
    S = env.observation_space.n
    obs = np.concatenate([c.obs.cpu().numpy() for c in traj_chunks], axis=1)
    act = np.concatenate([c.actions.cpu().numpy() for c in traj_chunks], axis=1)
    rew = np.concatenate([c.rewards.cpu().numpy() for c in traj_chunks], axis=0)
    done = np.concatenate([c.dones.cpu().numpy() for c in traj_chunks], axis=0)
    assert set(np.unique(obs)) <= {0.0, 1.0} and np.all(obs.sum(axis=0) == 1) and np.all(act.sum(axis=0) == 1)
    T = rew.shape[0]
    states, tss = [], []
    for i in range(n):
        s, ts = env.reset(), 0
        for t in range(T):
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


@pytest.mark.parametrize("desc", ["4x4", "4x4_safe", "chain"])
def test_rollout_replays_on_the_host_env(desc):
    n, T, L = 70, 40, 11                     # one full wavefront plus 6 lanes; paths end inside and across the launches
    env, pol = _grid_policy(desc)
    ve = env.vec_env_executor(n, L, seed=3)
    assert ve.takes_rollout_of(pol) and ve.n == n
    S = env.observation_space.n
    rng = np.random.RandomState(7)
    u = np.minimum(rng.rand(T + 13, n).astype(np.float32), np.float32(1 - 2.0 ** -24))
    table = pol.prob_table()
    assert table.shape == (4, S) and table.dtype == torch.float32
    first = ve.rollout(pol, T, reset_at_start=True, u=u[:T])
    assert first.categorical and first.log_std is None and (first.T, first.N, first.obs_dim, first.act_dim) == (T, n, S, 4)
    assert ve.step_counter == T
    states, tss = _replay(env, [first], n, L)
    assert ve.state.cpu().tolist() == states and ve.ts.cpu().tolist() == tss
    # recorded prob: the table column of the recorded state, bit for bit; recorded action: the cumulative rule in float32
    tab, prob = table.cpu().numpy(), first.means.cpu().numpy()
    s_idx = first.obs.cpu().numpy().argmax(axis=0)                         # [T, n]
    assert np.array_equal(prob, tab[:, s_idx])
    assert prob.dtype == np.float32 and np.cumsum(prob, axis=0).dtype == np.float32
    want = np.minimum((np.cumsum(prob, axis=0) < u[:T][None]).sum(axis=0), 3)
    assert np.array_equal(first.actions.cpu().numpy().argmax(axis=0), want)
    assert len(np.unique(want)) == 4 and first.dones.sum() > n            # every action taken, every env ended paths
    # a second launch without a reset continues each env where the first one ended
    second = ve.rollout(pol, 13, reset_at_start=False, u=u[T:])
    assert ve.step_counter == T + 13
    states, tss = _replay(env, [first, second], n, L)
    assert ve.state.cpu().tolist() == states and ve.ts.cpu().tolist() == tss
    # the plain VecEnv API on the same executor: a host loop over the Python env
    obs = ve.reset()
    assert obs == [env.start_state] * n and ve.ts.sum().item() == 0
    obs, rews, dones, _ = ve.step([2] * n)
    e = type(env)(desc)
    e.reset()
    assert obs == [e.step(2).observation] * n and rews.shape == (n,) and not dones.any()


@pytest.mark.parametrize("hidden", [(32, 32), (20,), (100, 50, 25)])
def test_table_is_the_float64_forward(hidden):
    env, pol = _grid_policy("4x4", hidden, seed=2)
    assert pol.kernel_net() is not None and pol.why_no_kernel_layout() is None
    table = pol.prob_table()
    eye = torch.eye(16, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        want = pol.dist_info_planes(eye, pol.flat_params.double())["prob"]
    assert float((table.double() - want).abs().max()) <= 1e-5
    assert float((table.double().sum(dim=0) - 1).abs().max()) <= 1e-6
    assert pol.prob_table() is table                                      # cached per parameter version
    pol.set_param_values(pol.get_param_values() + 0.05)
    assert pol.prob_table() is not table


def test_table_of_a_network_the_kernels_do_not_run():
    """'8x8' has 64 inputs: the table comes from the policy's own torch forward, the rollout kernel is the same."""
    env, pol = _grid_policy("8x8")
    assert pol.kernel_net() is None and pol.fused_ops() is None
    table = pol.prob_table()
    eye = torch.eye(64, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        want = pol.dist_info_planes(eye, pol.flat_params.double())["prob"]
    assert table.shape == (4, 64) and float((table.double() - want).abs().max()) <= 1e-5
    ve = env.vec_env_executor(70, 30, seed=1)
    traj = ve.rollout(pol, 30)
    _replay(env, [traj], 70, 30)


# -- the Philox path --------------------------------------------------------------------------------------------------
def test_philox_rollout_is_a_function_of_seed_and_counter():
    env, pol = _grid_policy("4x4")
    a, b, c = (env.vec_env_executor(200, 20, seed=5) for _ in range(3))
    c.step_counter = 1000
    ta, tb, tc = a.rollout(pol, 25), b.rollout(pol, 25), c.rollout(pol, 25)
    for name in ("obs", "actions", "means", "rewards", "dones"):
        assert torch.equal(getattr(ta, name), getattr(tb, name)), name
    assert not torch.equal(ta.actions, tc.actions)
    d = env.vec_env_executor(200, 20, seed=6).rollout(pol, 25)
    assert not torch.equal(ta.actions, d.actions)
    # env_offset shifts the streams: envs 100 .. 199 of one executor are envs 0 .. 99 of one that starts at 100
    e = env.vec_env_executor(100, 20, seed=5, env_offset=100).rollout(pol, 25)
    assert torch.equal(e.actions, ta.actions[:, :, 100:])


def test_philox_first_step_frequencies():
    """A five-sigma condition on a correct sampler at one fixed seed: |freq - p| <= 5 sqrt(p (1 - p) / n)."""
    n = 65536
    env, pol = _grid_policy("4x4", seed=4)
    ve = env.vec_env_executor(n, 10, seed=12345)
    traj = ve.rollout(pol, 1)
    p = pol.prob_table()[:, env.start_state].double().cpu().numpy()
    freq = traj.actions[:, 0, :].double().mean(dim=1).cpu().numpy()
    for k in range(4):
        assert abs(freq[k] - p[k]) <= 5 * np.sqrt(p[k] * (1 - p[k]) / n), (k, freq[k], p[k])


# -- head and Fisher kernels under the networks ------------------------------------------------------------------------
@pytest.mark.parametrize("do,da,hidden", NETWORKS)
@pytest.mark.parametrize("B", BATCHES)
def test_loss_kl_grad_vs_float64_autograd(do, da, hidden, B):
    pol = _policy(do, da, hidden)
    ops = pol.fused_ops()
    assert ops is not None and type(ops).__name__ == "FusedCategoricalOps"
    inp = _inputs(pol, B)
    assert ops.accepts(inp) and _min_prob(pol, inp) >= 1e-3
    surr, kl, vpg = _closures(pol)
    flat64 = pol.flat_params.detach().double().requires_grad_(True)
    l64, k64, v64 = surr(flat64, *inp), kl(flat64, *inp), vpg(flat64, *inp)
    s = ops.loss_stats(inp)
    print("loss", float(-s[0]), float(l64.detach()), "kl", float(s[1]), float(k64.detach()), "vpg", float(-s[2]), float(v64.detach()))
    assert abs(float(-s[0]) - float(l64.detach())) <= 2e-5 * max(1.0, abs(float(l64.detach())))
    assert abs(float(s[1]) - float(k64.detach())) <= 2e-5 * max(1e-2, abs(float(k64.detach())))
    assert abs(float(-s[2]) - float(v64.detach())) <= 2e-5 * max(1.0, abs(float(v64.detach())))
    with torch.no_grad():
        new = pol.dist_info_planes(inp[0].double(), pol.flat_params.double())
        kls = pol.distribution.kl_sym(dict(prob=inp[3].double()), new, axis=0)
        max_kl = float(torch.where(inp[4] > 0, kls, torch.full_like(kls, -float("inf"))).max())
    assert abs(float(s[3]) - max_kl) <= 2e-5 * max(1e-2, abs(max_kl))
    g64 = torch.autograd.grad(l64, flat64, retain_graph=True)[0]
    g = ops.loss_grad(inp)
    print("grad err", float((g - g64).abs().max()), "max", float(g64.abs().max()))
    assert g.shape == g64.shape and float((g - g64).abs().max()) <= 2e-5 * max(1e-3, float(g64.abs().max()))
    # two calls are bit-identical; the gradient pass hands back the same loss sums
    ops.release()
    g2 = ops.loss_grad(inp, with_loss=True)
    assert torch.equal(g2, g)
    assert torch.equal(ops.loss_stats(inp), s)
    gv64 = torch.autograd.grad(v64, flat64, retain_graph=True)[0]
    gv = ops.loss_grad(inp, vpg=True)
    assert float((gv - gv64).abs().max()) <= 2e-5 * max(1e-3, float(gv64.abs().max()))
    # PPO's penalised objective in one pass
    pen = 3.0
    val, gp = ops.value_and_grad(inp, pen)
    gk64 = torch.autograd.grad(k64, flat64)[0]
    want = float(l64.detach() + pen * k64.detach())
    assert abs(val - want) <= 2e-5 * max(1.0, abs(want))
    gp64 = (g64 + pen * gk64).cpu().numpy()
    assert np.abs(gp - gp64).max() <= 2e-5 * max(1e-3, np.abs(gp64).max())


@pytest.mark.parametrize("do,da,hidden", NETWORKS)
@pytest.mark.parametrize("B", BATCHES)
def test_fvp_equals_kl_hessian_at_theta_old(do, da, hidden, B):
    """The product against the double backward of the mean KL at old == new."""
    pol = _policy(do, da, hidden)
    ops = pol.fused_ops()
    inp = _inputs(pol, B, old_equals_new=True)
    assert _min_prob(pol, inp) >= 1e-3
    _, kl, _ = _closures(pol)
    rng = np.random.RandomState(3)
    flat64 = pol.flat_params.detach().double().requires_grad_(True)
    with torch.no_grad():
        old64 = pol.dist_info_planes(inp[0].double(), flat64.detach())["prob"]
    inp64 = (inp[0], inp[1], inp[2], old64, inp[4], inp[5])
    g = torch.autograd.grad(kl(flat64, *inp64), flat64, create_graph=True)[0]
    for trial in range(2):
        v = torch.as_tensor(rng.randn(flat64.numel()), device=flat64.device)
        hv64 = torch.autograd.grad((g * v).sum(), flat64, retain_graph=True)[0]
        hv = ops.fvp(inp, v)
        print("fvp err", float((hv - hv64).abs().max()), "max", float(hv64.abs().max()))
        assert float((hv - hv64).abs().max()) <= 5e-5 * float(hv64.abs().max())
        assert torch.equal(ops.fvp(inp, v), hv)                            # two calls are bit-identical
    # symmetric: u . F v == v . F u
    u = torch.as_tensor(rng.randn(flat64.numel()), device=flat64.device)
    v = torch.as_tensor(rng.randn(flat64.numel()), device=flat64.device)
    a, b = float(u.dot(ops.fvp(inp, v))), float(v.dot(ops.fvp(inp, u)))
    assert abs(a - b) <= 1e-4 * max(abs(a), abs(b))


@pytest.mark.parametrize("do,da,hidden", NETWORKS)
def test_device_cg_is_krylov_cg_on_the_products(do, da, hidden):
    from rllab_amd.misc import krylov
    pol = _policy(do, da, hidden)
    ops = pol.fused_ops()
    inp = _inputs(pol, 3000, old_equals_new=True)
    g = ops.loss_grad(inp)
    x, xhx = ops.cg(inp, g, 5, 1e-5)
    want = krylov.cg(lambda p: ops.fvp(inp, p) + 1e-5 * p, g, cg_iters=5)
    assert float((x - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert float(xhx) > 0


@pytest.mark.parametrize("do,da,hidden", NETWORKS)
def test_zero_weights_contribute_nothing(do, da, hidden):
    """A batch whose last third has weight 0 gives the sums and the gradient of the first two thirds alone.  The head's
    sums are float64 (reordered: 1e-12 relative); the network's backward pass adds float32 products per tile, the zero
    cotangents of the masked tiles add exact zeros, and what may differ is the order in which the workgroups' float32
    partial rows are taken: 6e-8 sqrt(2000) < 1e-5 relative to the largest entry."""
    B = 3000
    pol = _policy(do, da, hidden)
    ops = pol.fused_ops()
    obs, act, adv, op, w, _ = _inputs(pol, B, ragged=False)
    w = w.clone()
    w[2 * B // 3:] = 0.0
    inv = 1.0 / w.double().sum()
    full = (obs, act, adv, op, w, inv)
    k = 2 * B // 3
    part = (obs[:, :k].contiguous(), act[:, :k].contiguous(), adv[:k].contiguous(), op[:, :k].contiguous(),
            w[:k].contiguous(), inv)
    s_full, g_full = ops.loss_stats(full).clone(), ops.loss_grad(full).clone()
    v = torch.as_tensor(np.random.RandomState(9).randn(g_full.numel()), device="cuda")
    h_full = ops.fvp(full, v).clone()
    ops.release()
    s_part, g_part, h_part = ops.loss_stats(part), ops.loss_grad(part), ops.fvp(part, v)
    assert torch.allclose(s_full, s_part, rtol=1e-12, atol=1e-15)
    assert float((g_full - g_part).abs().max()) <= 1e-5 * float(g_part.abs().max())
    assert float((h_full - h_part).abs().max()) <= 1e-5 * float(h_part.abs().max())


# -- the head kernels alone, on random logit planes ----------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 4, 8])
@pytest.mark.parametrize("B", [1, 63, 70001, 300001])      # 300001: past 1024 workgroups of 256, the grid-stride loop
def test_head_kernels_on_random_logits(A, B):
    from rllab_amd import _lib
    from rllab_amd.distributions.categorical import Categorical
    dist = Categorical(A)
    rng = np.random.RandomState(A * 1000 + B % 997)
    dev = "cuda"
    logits = torch.as_tensor((0.5 * rng.randn(A, B)).astype(np.float32), device=dev)
    old = torch.softmax(logits.double() + 0.05 * torch.as_tensor(rng.randn(A, B), device=dev), dim=0).float()
    assert float(old.min()) >= 1e-3 and float(torch.softmax(logits.double(), dim=0).min()) >= 1e-3
    idx = torch.as_tensor(rng.randint(0, A, size=B), device=dev)
    act = torch.nn.functional.one_hot(idx, A).t().float().contiguous()
    adv = torch.as_tensor(rng.randn(B).astype(np.float32), device=dev)
    w = torch.as_tensor((rng.rand(B) >= 0.1).astype(np.float32), device=dev)
    w[0] = 1.0
    inv = float(1.0 / w.double().sum())
    ws = torch.empty(_lib.lib.rl_categorical_head_workspace_bytes(), dtype=torch.uint8, device=dev)

    def head(vpg, pen, want_g):
        out4 = torch.empty(4, dtype=torch.float64, device=dev)
        g = torch.empty((A, B), dtype=torch.float32, device=dev) if want_g else None
        _lib.check(_lib.lib.rl_categorical_head(B, A, _lib.ptr(logits), _lib.ptr(act), _lib.ptr(adv), _lib.ptr(old),
                                                _lib.ptr(w), inv, vpg, pen, _lib.ptr(g), _lib.ptr(ws), ws.numel(),
                                                _lib.ptr(out4), _lib.stream_ptr()), "rl_categorical_head")
        return out4, g

    z = logits.double().requires_grad_(True)
    new = dict(prob=torch.softmax(z, dim=0))
    o = dict(prob=old.double())
    lr = dist.likelihood_ratio_sym(act.double(), o, new, axis=0)
    kl = dist.kl_sym(o, new, axis=0)
    logp = dist.log_likelihood_sym(act.double(), new, axis=0)
    wd, ad = w.double(), adv.double()
    sums = [(wd * lr * ad).sum(), (wd * kl).sum(), (wd * logp * ad).sum()]
    out4, none = head(0, 0.0, False)
    assert none is None
    for got, want in zip(out4[:3].tolist(), sums):
        assert abs(got - float(want)) <= 2e-5 * max(1.0, abs(float(want)))
    assert abs(float(out4[3]) - float(kl[w > 0].max())) <= 2e-5 * max(1e-2, float(kl[w > 0].max()))
    for vpg, pen in ((0, 0.0), (1, 0.0), (0, 2.5)):
        obj = (-(sums[2] if vpg else sums[0]) + pen * sums[1]) * inv
        g64 = torch.autograd.grad(obj, z, retain_graph=True)[0]
        out4b, g = head(vpg, pen, True)
        assert torch.equal(out4b, out4)
        assert float((g.double() - g64).abs().max()) <= 2e-5 * float(g64.abs().max())
        assert torch.equal(head(vpg, pen, True)[1], g)                     # bit-identical
        assert float(g[:, w == 0].abs().max() if bool((w == 0).any()) else 0.0) == 0.0
    # Fisher: the Hessian of the per-sample KL in the logits at new == old, TINY kept
    dz = torch.as_tensor(rng.randn(A, B).astype(np.float32), device=dev)
    p_old = torch.softmax(logits.double(), dim=0)
    kl0 = (dist.kl_sym(dict(prob=p_old), new, axis=0) * wd).sum() * inv
    g1 = torch.autograd.grad(kl0, z, create_graph=True)[0]
    hv64 = torch.autograd.grad((g1 * dz.double()).sum(), z)[0]
    hv = torch.empty((A, B), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib.rl_categorical_fisher(B, A, _lib.ptr(dz), _lib.ptr(logits), _lib.ptr(w), inv, _lib.ptr(hv),
                                              _lib.stream_ptr()), "rl_categorical_fisher")
    assert float((hv.double() - hv64).abs().max()) <= 5e-5 * float(hv64.abs().max())
    assert float(hv[:, w == 0].abs().max() if bool((w == 0).any()) else 0.0) == 0.0
    # softmax planes
    prob = torch.empty((A, B), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib.rl_categorical_softmax(B, A, _lib.ptr(logits), _lib.ptr(prob), _lib.stream_ptr()), "softmax")
    assert float((prob.double() - p_old).abs().max()) <= 1e-7


def test_argument_errors_launch_nothing():
    from rllab_amd import _lib
    lib = _lib.lib
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    i8 = torch.zeros(16, dtype=torch.int8, device="cuda")
    p = lambda t: t.data_ptr()

    def grid(**kw):
        a = dict(n_envs=2, horizon=2, max_path_length=5, reset_at_start=1, n_row=4, n_col=4, n_act=4, start_state=0,
                 cell=p(i8), prob=p(x), state=p(i32), ts=p(i32), obs=p(x), actions=p(x), prob_out=p(x), rewards=p(x),
                 dones=p(i8))
        a.update(kw)
        return lib.rl_rollout_gridworld(ctypes.byref(_lib.GridWorldArgs(**a)), None)

    for kw, word in ((dict(prob=None), "null"), (dict(cell=None), "null"), (dict(n_act=9), "n_act 9"),
                     (dict(n_envs=0), "zero-sized"), (dict(horizon=0), "zero-sized"), (dict(n_row=40, n_col=40), "states"),
                     (dict(start_state=16), "start_state")):
        assert grid(**kw) == -1 and word in lib.rl_last_error().decode(), kw
    assert lib.rl_rollout_gridworld(None, None) == -1
    ws = torch.empty(lib.rl_categorical_head_workspace_bytes(), dtype=torch.uint8, device="cuda")
    out4 = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    v = _lib.ptr

    def head(B=8, A=4, logits=x, ws_bytes=None):
        return lib.rl_categorical_head(B, A, v(logits), v(x), v(x), v(x), v(x), 1.0, 0, 0.0, None, v(ws),
                                       ws.numel() if ws_bytes is None else ws_bytes, v(out4), None)
    assert head(logits=None) == -1 and "null" in lib.rl_last_error().decode()
    assert head(A=9) == -1 and "n_act 9" in lib.rl_last_error().decode()
    assert head(B=0) == -1 and "n_samples 0" in lib.rl_last_error().decode()
    assert head(ws_bytes=8) == -1 and "workspace" in lib.rl_last_error().decode()
    assert lib.rl_categorical_fisher(8, 9, v(x), v(x), v(x), 1.0, v(x), None) == -1
    assert lib.rl_categorical_fisher(0, 4, v(x), v(x), v(x), 1.0, v(x), None) == -1
    assert lib.rl_categorical_fisher(8, 4, None, v(x), v(x), 1.0, v(x), None) == -1
    assert lib.rl_categorical_softmax(8, 9, v(x), v(x), None) == -1 and lib.rl_categorical_softmax(0, 4, v(x), v(x), None) == -1
    torch.cuda.synchronize()
    assert torch.all(out4 == 7.0) and torch.all(x == 0)                    # nothing was launched


# -- the reference's matrix: every algorithm on GridWorld with a categorical MLP --------------------------------------
def _algo(name, env, policy, **kw):
    import importlib
    from rllab_amd.baselines.linear_feature_baseline import LinearFeatureBaseline
    cls = getattr(importlib.import_module("rllab_amd.algos." + name.lower()), name)
    args = dict(env=env, policy=policy, baseline=LinearFeatureBaseline(env_spec=env.spec), batch_size=1000,
                max_path_length=100, n_itr=1)
    if name in ("TRPO", "TNPG"):
        args["optimizer_args"] = dict(cg_iters=1)
    args.update(kw)
    return cls(**args)


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


@pytest.mark.parametrize("name", ["TRPO", "TNPG", "VPG", "PPO"])
def test_algorithms_on_gridworld(name, tmp_path):
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
    ext.set_seed(1)
    env = GridWorldEnv()
    policy = CategoricalMLPPolicy(env_spec=env.spec)
    theta0 = policy.get_param_values()
    algo = _algo(name, env, policy)
    text, rows = _train_logged(algo, tmp_path)
    theta = policy.get_param_values()
    assert np.all(np.isfinite(theta)) and theta.shape == theta0.shape
    assert "sampling path: fused rollout kernel" in text
    assert "update path: HIP kernels (FusedCategoricalOps)" in text
    assert len(rows) == 1 and int(rows[0]["NumTrajs"]) > 0
    ent = float(rows[0]["Entropy"])
    assert 0 < ent <= -np.log(0.25 + 1e-8) + 1e-6 and abs(float(rows[0]["Perplexity"]) - np.exp(ent)) < 1e-9
    assert "AveragePolicyStd" not in rows[0]                               # nothing Gaussian is logged
    assert algo.sampler.last_num_samples >= 1000


def test_8x8_samples_on_the_kernel_and_updates_through_autograd(tmp_path):
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
    ext.set_seed(1)
    env = GridWorldEnv("8x8")
    policy = CategoricalMLPPolicy(env_spec=env.spec)
    text, rows = _train_logged(_algo("TRPO", env, policy), tmp_path)
    assert np.all(np.isfinite(policy.get_param_values()))
    assert "sampling path: fused rollout kernel" in text
    assert "update path: torch autograd -- " in text and "64" in text.split("update path: torch autograd -- ")[1].split("\n")[0]
    assert len(rows) == 1


@pytest.mark.parametrize("name", ["ERWR", "REPS", "CEM"])
def test_algorithms_without_a_categorical_path_say_so(name):
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import logger
    from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
    env = GridWorldEnv()
    policy = CategoricalMLPPolicy(env_spec=env.spec)
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


def test_trpo_learns_gridworld(tmp_path):
    """TRPO on '4x4', 15 iterations of 4000 samples.  Every iteration: MeanKL <= 0.0101, LossAfter < LossBefore,
    |MeanKLBefore| < 1e-6.  The return: the mean of the last three iterations exceeds the mean of the first three by at
    least half the gain of the same configuration on the CPU (tools/exp/trpo_gridworld_cpu.py: the Python env sampled one
    path after another, float64 autograd update; profiles/curves/trpo_gridworld_cpu.csv) -- half is the margin for the
    two samplers' different random streams."""
    from rllab_amd.algos.trpo import TRPO
    from rllab_amd.baselines.linear_feature_baseline import LinearFeatureBaseline
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
    with open(os.path.join(ROOT, "profiles", "curves", "trpo_gridworld_cpu.csv")) as f:
        cpu = [float(r["AverageReturn"]) for r in csv.DictReader(f)]
    assert len(cpu) == 15
    cpu_gain = np.mean(cpu[-3:]) - np.mean(cpu[:3])
    assert cpu_gain > 0.5
    ext.set_seed(1)
    env = GridWorldEnv("4x4")
    policy = CategoricalMLPPolicy(env_spec=env.spec)
    algo = TRPO(env=env, policy=policy, baseline=LinearFeatureBaseline(env_spec=env.spec), batch_size=4000,
                max_path_length=50, n_itr=15, discount=0.99, step_size=0.01)
    text, rows = _train_logged(algo, tmp_path)
    assert "update path: HIP kernels (FusedCategoricalOps)" in text and len(rows) == 15
    ret = [float(r["AverageReturn"]) for r in rows]
    print("AverageReturn", ret)
    for r in rows:
        print(r["Iteration"], r["LossBefore"], r["LossAfter"], r["MeanKLBefore"], r["MeanKL"])
    for r in rows:
        assert float(r["MeanKL"]) <= 0.0101, r
        assert float(r["LossAfter"]) < float(r["LossBefore"]), r
        assert abs(float(r["MeanKLBefore"])) < 1e-6, r
    assert np.mean(ret[-3:]) - np.mean(ret[:3]) >= 0.5 * cpu_gain, (ret, cpu_gain)
