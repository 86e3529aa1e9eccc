"""The recurrent update kernels (rl_gru_gaussian_eval / _grad / _fvp, csrc/gru_bptt_kernels.hip) and TRPO / TNPG on them
(GaussianGRUPolicy(bptt_kernels=True), policies/fused_gru_ops.py).

Reference: the closures of algos/npo.py (restated below on ``policy.dist_info_planes`` and the policy's distribution)
differentiated by torch autograd in float64; yardstick: the same in float32, which is what the update runs without the
option.  The rule for every compared quantity: the kernel's relative error against float64 is at most 8 x the float32
autograd's, the yardstick floored at 2^-20.  The kernel evaluates sigmoid and tanh on the hardware's rcp / exp2 and sums
sequentially, torch calls library functions and sums in blocks, both carry the same amplification through T steps: 8 is
an allowance for that, not a measurement (the measured ratios are printed, and listed in DESIGN section 3.17).

Shapes: N = 70 (a partial second wavefront), T = 25 with a start in the last row, two consecutive starts, columns without
a start after row 0 and trailing weights = 0; T = 1; N = 1.  (13, 2) at 64 units and (20, 6) at 64 units do not fit the
LDS of a CU next to their tangent vector: those two are the refusal cases.
"""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -20
ALLOW = 8.0
# (env kind -> (Do, Da): 0 (4, 1), 2 (13, 2), 3 (20, 6)), hidden, N, T, include_action
CASES = [(0, 20, 70, 25, True), (0, 32, 70, 25, True), (0, 64, 70, 25, True), (2, 20, 70, 25, True), (2, 32, 70, 25, True),
         (3, 32, 70, 25, True), (2, 32, 70, 25, False), (0, 32, 70, 1, True), (0, 32, 1, 25, True)]


def _policy(kind, hidden, seed=0, scale=0.1, **kw):
    """A GaussianGRUPolicy(bptt_kernels=True) for env ``kind`` with every parameter -- h0, the biases and log_std too --
    moved off its initial value."""
    from rllab_amd import _lib
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.spaces import Box
    q = _lib.env_query(kind)
    spec = EnvSpec(Box(-1e6 * np.ones(q["obs_dim"]), 1e6 * np.ones(q["obs_dim"])),
                   Box(-np.ones(q["act_dim"]), np.ones(q["act_dim"])))
    np.random.seed(seed)
    kw.setdefault("bptt_kernels", True)
    pol = GaussianGRUPolicy(spec, hidden_sizes=(hidden,), **kw)
    theta = pol.get_param_values()
    pol.set_param_values(theta + scale * np.random.RandomState(seed + 1).randn(theta.size))
    return pol


def _planes(pol, N, T, seed=3, at_old=False, obs_scale=1.0, edit=None):
    """Synthetic planes in the order of npo_inputs.  ``at_old``: old == new (the point the Fisher matrix is taken at);
    else the old means are the current ones plus a perturbation and the old log_std is moved: lr != 1, KL != 0.
    ``obs_scale`` multiplies the observation planes; ``edit(start, w)`` changes the start mask and the weights in place
    (numpy, [T, N]) behind the columns made here; neither draws from the generator."""
    rng = np.random.RandomState(seed)
    dev = pol.flat_params.device
    f = lambda *s: torch.as_tensor(rng.randn(*s).astype(np.float32), device=dev)
    Do, Da = pol.obs_dim, pol.action_dim
    obs, act, adv = obs_scale * f(Do, T, N), 0.5 * f(Da, T, N), f(T, N)
    start = rng.rand(T, N) < 0.08
    w = np.ones((T, N), dtype=np.float32)
    start[0] = True
    if T >= 25:
        start[:, 2 % N] = False                   # columns with no start after row 0
        start[:, N - 1] = False
        start[5:7, 0] = True                      # two consecutive starts: a path of length 1
        start[T - 1, 1 % N] = True                # a start in the last row
        start[18, 3 % N] = True                   # trailing weights = 0 segments (the rows behind a path that ended)
        w[20:, 3 % N] = 0.0
        w[T - 2:, 5 % N] = 0.0
        start[0] = True
    if edit is not None:
        edit(start, w)
        start[0] = True
    start = torch.as_tensor(start, device=dev)
    w = torch.as_tensor(w, device=dev)
    with torch.no_grad():
        d = pol.dist_info_planes(obs, act, start)
    ls = d["log_std"].reshape(-1, 1, 1).clone()
    if at_old:
        old_mean, old_ls = d["mean"].clone(), ls
    else:
        old_mean, old_ls = d["mean"] + 0.05 * f(Da, T, N), ls + 0.05 * f(Da, 1, 1)
    inv = 1.0 / w.double().sum().cpu()
    return (obs, act, adv, old_mean.contiguous(), old_ls, start, w, inv)


def _closures(pol):
    """algos/npo.py's recurrent closures."""
    dist = pol.distribution

    def surr_loss(flat, obs, act, adv, old_mean, old_log_std, start, w, inv_count):
        new = pol.dist_info_planes(obs, act, start, flat)
        lr = dist.likelihood_ratio_sym(act, dict(mean=old_mean, log_std=old_log_std), new, axis=0)
        return -(lr * adv * w).sum() * inv_count.to(lr.dtype)

    def mean_kl(flat, obs, act, adv, old_mean, old_log_std, start, w, inv_count):
        new = pol.dist_info_planes(obs, act, start, flat)
        kl = dist.kl_sym(dict(mean=old_mean, log_std=old_log_std), new, axis=0)
        return (kl * w).sum() * inv_count.to(kl.dtype)
    return surr_loss, mean_kl


def _cast(inputs, dt):
    return tuple(x.to(dt) if torch.is_tensor(x) and x.is_floating_point() else x for x in inputs)


def _grad(pol, fn, inputs, dt):
    flat = pol.flat_params.detach().to(dt).requires_grad_(True)
    val = fn(flat, *_cast(inputs, dt))
    return val.detach().double(), torch.autograd.grad(val, flat)[0].double()


def _hvp(pol, fn, inputs, dt, vs):
    """PerlmutterHvp's double back-propagation, for every direction of ``vs`` on one graph."""
    flat = pol.flat_params.detach().to(dt).requires_grad_(True)
    g = torch.autograd.grad(fn(flat, *_cast(inputs, dt)), flat, create_graph=True)[0]
    return [torch.autograd.grad((g * v.to(dt)).sum(), flat, retain_graph=True)[0].double() for v in vs]


def _rel(x, ref):
    return float((x - ref).norm() / ref.norm())


def _within(name, got, ref64, ref32):
    e_k, e_32 = _rel(got, ref64), _rel(ref32, ref64)
    print("%s: kernel %.3e, float32 autograd %.3e, ratio to the floored yardstick %.2f" % (
        name, e_k, e_32, e_k / max(e_32, FLOOR)))
    assert e_k <= ALLOW * max(e_32, FLOOR), name


_REF = {}


def _case(case):
    """Policy, ops, planes and the autograd references of a case, computed once and shared (never written to)."""
    if case in _REF:
        return _REF[case]
    kind, hidden, N, T, inc = case
    pol = _policy(kind, hidden, state_include_action=inc)
    ops = pol.fused_ops()
    assert ops is not None, pol.why_no_kernel_layout()
    inputs = _planes(pol, N, T)
    surr, kl = _closures(pol)
    r = dict(pol=pol, ops=ops, inputs=inputs, idx=pol._flat_index(trainable=True))
    r["l64"], r["g64"] = _grad(pol, surr, inputs, torch.float64)
    r["l32"], r["g32"] = _grad(pol, surr, inputs, torch.float32)
    with torch.no_grad():
        r["k64"] = kl(pol.flat_params.detach().double(), *_cast(inputs, torch.float64)).double()
        r["k32"] = kl(pol.flat_params.detach(), *inputs).double()
    _REF[case] = r
    return r


# -- 1. the forward sweep is the rollout's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [32, 20, 64])
def test_forward_sweep_reproduces_the_rollouts_means(hidden):
    from rllab_amd.envs.hip_env import HipVecEnv
    N, T, MPL = 70, 25, 11
    pol = _policy(0, hidden)
    v = HipVecEnv(0, N, MPL, normalize=True, seed=5)
    assert v.takes_rollout_of(pol)
    traj = v.rollout(pol, T)
    assert int(traj.dones.sum()) > 0
    start = torch.ones_like(traj.dones, dtype=torch.bool)
    start[1:] = traj.dones[:-1].bool()
    adv = torch.randn(T, N, device=traj.device)
    w = torch.ones(T, N, device=traj.device)
    inputs = (traj.obs, traj.actions, adv, traj.means, traj.log_std.reshape(-1, 1, 1), start, w,
              torch.tensor(1.0 / (T * N), dtype=torch.float64))
    ops = pol.fused_ops()
    assert ops.accepts(inputs)
    assert torch.equal(ops.forward_means(inputs), traj.means)
    assert torch.equal(ops.forward_means(inputs, with_grad=True), traj.means)
    ops.release()
    loss, kl = ops.loss_and_kl(inputs)
    assert kl == 0.0 and np.isfinite(loss)          # kl_sym's terms vanish identically at equal inputs


# -- 2., 4., 6. gradient, sums, padding ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_gradient_and_sums_against_autograd(case):
    r = _case(case)
    pol, ops, inputs, idx = r["pol"], r["ops"], r["inputs"], r["idx"]
    ops.release()
    l_e, k_e = ops.loss_and_kl(inputs)
    ops.release()
    gk = ops.loss_grad_kernel(inputs, with_loss=True)
    l_g, k_g = ops.loss_and_kl(inputs)                   # (the record the gradient pass left)
    assert (l_e, k_e) == (l_g, k_g)                      # EVAL and GRAD: the same bits
    t = lambda x: torch.as_tensor([x], dtype=torch.float64)
    _within("loss %r" % (case,), t(l_e), r["l64"].cpu().reshape(1), r["l32"].cpu().reshape(1))
    _within("KL %r" % (case,), t(k_e), r["k64"].cpu().reshape(1), r["k32"].cpu().reshape(1))
    assert k_e > 0
    g = ops.gather(gk).double()
    _within("gradient %r" % (case,), g[idx], r["g64"][idx], r["g32"][idx])
    # h0 is not trainable; the padded places of the kernel layout hold exact zeros
    H = pol.kernel_hidden
    assert bool(torch.all(gk[:H] == 0))
    pad = torch.ones(ops.n_kernel, dtype=torch.bool, device=gk.device)
    if ops.index is not None:
        pad[ops.index] = False
        assert int(pad.sum()) == ops.n_kernel - ops.n_flat > 0 and bool(torch.all(gk[pad] == 0))
    else:
        assert ops.n_kernel == ops.n_flat
    flat = ops.loss_grad(inputs)
    assert flat.dtype == torch.float64 and bool(torch.all(flat[:pol.hidden_dim] == 0))


def test_frozen_log_std_gets_exact_zeros():
    pol = _policy(0, 32, learn_std=False)
    ops = pol.fused_ops()
    inputs = _planes(pol, 70, 25)
    surr, _ = _closures(pol)
    idx = pol._flat_index(trainable=True)
    g = ops.loss_grad(inputs)
    assert bool(torch.all(g[-1:] == 0)) and bool(torch.all(g[:32] == 0))
    _, g64 = _grad(pol, surr, inputs, torch.float64)
    _, g32 = _grad(pol, surr, inputs, torch.float32)
    _within("gradient, learn_std=False", g[idx], g64[idx], g32[idx])


# -- 3. Fisher-vector product ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_fisher_vector_product_against_perlmutter(case):
    r = _case(case)
    pol, ops, idx = r["pol"], r["ops"], r["idx"]
    kind, hidden, N, T, inc = case
    inputs = _planes(pol, N, T, at_old=True)
    _, kl = _closures(pol)
    n = pol.flat_params.numel()
    dev = pol.flat_params.device
    rng = np.random.RandomState(11)

    def direction(x):
        v = torch.zeros(n, dtype=torch.float64, device=dev)
        v[idx] = x[idx]
        return v
    u = direction(torch.as_tensor(rng.randn(n), device=dev))
    v = direction(torch.as_tensor(rng.randn(n), device=dev))
    g = direction(r["g64"])
    ops.release()
    Fu, Fv, Fg = (ops.fvp(inputs, x) for x in (u, v, g))
    H64 = _hvp(pol, kl, inputs, torch.float64, (u, v, g))
    H32 = _hvp(pol, kl, inputs, torch.float32, (u, v, g))
    for name, got, x, h64, h32 in (("u", Fu, u, H64[0], H32[0]), ("v", Fv, v, H64[1], H32[1]), ("g", Fg, g, H64[2], H32[2])):
        _within("F %s %r" % (name, case), got[idx], h64[idx], h32[idx])
        assert float(x.dot(got)) > 0
    # symmetry, to the same relative bound: |u'Fv - v'Fu| / |u'Fv| against what float32 autograd's two products give
    a, b = float(u.dot(Fv)), float(v.dot(Fu))
    a32, b32 = float(u.dot(H32[1])), float(v.dot(H32[0]))
    e_k, e_32 = abs(a - b) / abs(a), abs(a32 - b32) / abs(a32)
    print("u'Fv %.9e, v'Fu %.9e: asymmetry %.3e; float32 autograd %.9e, %.9e: %.3e; ratio to the floored yardstick %.2f" % (
        a, b, e_k, a32, b32, e_32, e_k / max(e_32, FLOOR)))
    assert e_k <= ALLOW * max(e_32, FLOOR)
    # the optimizer's plug-in: F x [idx] + reg x in float64
    hvp = ops.hvp_approach()
    hvp.update_opt(f=kl, target=pol, inputs=None, reg_coeff=1e-5)
    x = v[idx]
    got = hvp.build_eval(inputs, idx)(x)
    assert got.dtype == torch.float64 and torch.equal(got, Fv[idx] + 1e-5 * x)


# -- 5. determinism ------------------------------------------------------------------------------------------------------------
def test_every_pass_twice_gives_the_same_bits():
    r = _case(CASES[3])                                  # (13, 2) at 20 units: padding, two actions
    ops, inputs = r["ops"], r["inputs"]
    n = ops.n_kernel
    v = torch.as_tensor(np.random.RandomState(2).randn(n).astype(np.float32), device=inputs[0].device)
    v = ops.scatter(ops.gather(v))                       # zeros at the padded places
    ops.release()
    e1 = ops.loss_and_kl(inputs)
    ops.release()
    e2 = ops.loss_and_kl(inputs)
    assert e1 == e2
    g1 = ops.loss_grad_kernel(inputs).clone()
    s1 = ops._last_out2.clone()
    f1 = ops.fvp_kernel(inputs, v).clone()
    f2 = ops.fvp_kernel(inputs, v).clone()
    g2 = ops.loss_grad_kernel(inputs).clone()            # ... behind two products on the same workspace
    assert torch.equal(f1, f2) and torch.equal(g1, g2) and torch.equal(s1, ops._last_out2)
    assert torch.equal(ops.fvp_kernel(inputs, v), f1)
    assert float(g1.abs().max()) > 0 and float(f1.abs().max()) > 0 and bool(torch.isfinite(f1).all())


# -- 7. refusals -------------------------------------------------------------------------------------------------------------------
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
    args.update(kw)
    return cls(**args)


@pytest.mark.parametrize("case,sentence", [
    ("hidden", "hidden_sizes=(100,): the recurrent update kernels run 1 .. 64 hidden units"),
    ("rectify", "hidden_nonlinearity is rectify (the recurrent update kernels evaluate tanh)"),
    ("output", "output_nonlinearity is not None (the output layer of the recurrent update kernels is linear)")])
def test_policies_the_kernels_do_not_take_fall_back_to_autograd(case, sentence, tmp_path):
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    ext.set_seed(1)
    env = CartpoleEnv()
    kw = dict(hidden=dict(hidden_sizes=(100,)), rectify=dict(hidden_nonlinearity=rectify),
              output=dict(output_nonlinearity=torch.tanh))[case]
    policy = GaussianGRUPolicy(env_spec=env.spec, bptt_kernels=True, **kw)
    assert policy.fused_ops() is None and policy.why_no_kernel_layout() == sentence
    # (the fused rollout does not take these policies either, and a recurrent policy has no other sampling path: the
    # update path is decided, and logged, by init_opt)
    from rllab_amd.misc import logger
    algo = _algo("TRPO", env, policy, batch_size=200, max_path_length=20)
    txt = str(tmp_path / "log.txt")
    logger.add_text_output(txt)
    logger.set_quiet(True)
    try:
        algo.init_opt()
    finally:
        logger.remove_text_output(txt)
        logger.set_quiet(False)
    assert "update path: torch autograd -- " + sentence in open(txt).read()
    assert algo.optimizer._fused is None


@pytest.mark.parametrize("obs_dim,act_dim", [(20, 6), (13, 2)])
def test_a_shape_over_the_lds_budget_launches_nothing(obs_dim, act_dim):
    from rllab_amd import _lib
    lib = _lib.lib
    N, T, H = 8, 3, 64
    dev = torch.device("cuda", 0)
    full = lambda *shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=dev)
    assert lib.rl_gru_workspace_bytes(N, T, obs_dim, act_dim, H, 1) == 0
    msg = lib.rl_last_error().decode()
    assert "bytes of LDS" in msg and int(msg.split(":")[1].split()[0]) > 160 * 1024
    out2, grad, ws, means = full(2, dtype=torch.float64), full(32768), full(1 << 20), full(act_dim, T, N)
    planes = dict(theta=full(32768), obs=full(obs_dim, T, N), actions=full(act_dim, T, N), advantages=full(T, N),
                  old_means=full(act_dim, T, N), old_log_std=full(act_dim), start=full(T, N, dtype=torch.uint8),
                  weights=full(T, N))
    b = _lib.GruBatch(n_envs=N, horizon=T, obs_dim=obs_dim, act_dim=act_dim, hidden=H, include_action=1, inv_count=1.0,
                      means=means.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 4,
                      **{k: t.data_ptr() for k, t in planes.items()})
    assert lib.rl_gru_gaussian_eval(ctypes.byref(b), out2.data_ptr(), None) == -2
    assert "bytes of LDS" in lib.rl_last_error().decode()
    assert lib.rl_gru_gaussian_grad(ctypes.byref(b), out2.data_ptr(), grad.data_ptr(), None) == -2
    assert lib.rl_gru_gaussian_fvp(ctypes.byref(b), planes["theta"].data_ptr(), grad.data_ptr(), None) == -2
    torch.cuda.synchronize()
    for name, t in dict(out2=out2, grad=grad, ws=ws, means=means).items():
        assert bool(torch.all(t == 7)), name                                   # nothing was launched
    # the policy says so and its update runs through autograd
    pol = _policy(2 if obs_dim == 13 else 3, 64)
    assert pol.fused_ops() is None and "bytes of LDS" in pol.why_no_kernel_layout()


# -- 8. end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TRPO", "TNPG", "TRPO-fd", "VPG"])
def test_algorithms_on_cartpole_with_the_recurrent_kernels(name, tmp_path):
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    ext.set_seed(1)
    env = CartpoleEnv()
    policy = GaussianGRUPolicy(env_spec=env.spec, bptt_kernels=True)
    theta0 = policy.get_param_values()
    if name == "TRPO-fd":
        from rllab_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, FiniteDifferenceHvp
        algo = _algo("TRPO", env, policy, optimizer_args=None,
                     optimizer=ConjugateGradientOptimizer(cg_iters=1, hvp_approach=FiniteDifferenceHvp(base_eps=1e-5)))
    else:
        algo = _algo(name, env, policy)
    text, rows = _train_logged(algo, tmp_path)
    theta = policy.get_param_values()
    assert np.all(np.isfinite(theta)) and np.abs(theta - theta0).max() > 0
    assert np.array_equal(theta[:32], theta0[:32])                       # h0 is not trainable
    assert "sampling path: fused rollout kernel" in text and len(rows) == 1
    if name == "VPG":
        assert ("update path: torch autograd -- the recurrent kernels serve ConjugateGradientOptimizer (TRPO, TNPG)"
                in text)
        return
    assert "update path: HIP kernels (FusedGRUOps)" in text
    print(name, "MeanKLBefore", rows[0]["MeanKLBefore"], "MeanKL", rows[0]["MeanKL"], "dLoss", rows[0]["dLoss"])
    assert float(rows[0]["MeanKLBefore"]) == 0.0


# -- 9. learning ---------------------------------------------------------------------------------------------------------------------
def test_trpo_learns_cartpole_on_the_recurrent_kernels(tmp_path):
    """examples/trpo_gru_cartpole.py's configuration with --bptt-kernels (the optimizer's default products: the
    Fisher-vector kernel), seed 1, against the criteria of test_gpu_gru.py's learning test and its committed CPU
    yardstick: every iteration MeanKL <= 0.0101 and LossAfter < LossBefore; the mean return of the last three iterations
    exceeds that of the first three by at least half the yardstick's gain."""
    from examples.trpo_gru_cartpole import CONFIG, make_algo
    with open(os.path.join(ROOT, "profiles", "curves", "trpo_gru_cartpole_cpu.csv")) as f:
        cpu = [float(r["AverageReturn"]) for r in csv.DictReader(f)]
    assert len(cpu) == CONFIG["n_itr"]
    cpu_gain = np.mean(cpu[-3:]) - np.mean(cpu[:3])
    assert cpu_gain > 0
    text, rows = _train_logged(make_algo(seed=1, bptt_kernels=True), tmp_path)
    assert "update path: HIP kernels (FusedGRUOps)" in text and len(rows) == CONFIG["n_itr"]
    ret = [float(r["AverageReturn"]) for r in rows]
    print("AverageReturn", ret, "CPU", cpu)
    for r in rows:
        print(r["Iteration"], r["LossBefore"], r["LossAfter"], r["MeanKLBefore"], r["MeanKL"])
    for r in rows:
        assert float(r["MeanKLBefore"]) == 0.0, r
        assert float(r["MeanKL"]) <= 0.0101, r
        assert float(r["LossAfter"]) < float(r["LossBefore"]), r
    assert np.mean(ret[-3:]) - np.mean(ret[:3]) >= 0.5 * cpu_gain, (ret, cpu_gain)
