"""The recurrent categorical update kernels (rl_gru_categorical_eval / _grad / _fvp,
csrc/categorical_gru_bptt_kernels.hip) and TRPO / TNPG on them (CategoricalGRUPolicy(bptt_kernels=True),
policies/fused_categorical_gru_ops.py).

Reference: the recurrent categorical closures of algos/npo.py (restated below on ``policy.dist_info_planes`` and the policy's
distribution) differentiated by torch autograd in float64; yardstick: the same in float32, which is what the update runs
without the option.  The rule is tests/test_gpu_gru_bptt.py's, unchanged: for every compared quantity the kernel's relative
error against float64 is at most 8 x the float32 autograd's, the yardstick floored at 2^-20 (the measured ratios are
printed, and listed in DESIGN section 3.18).

Shapes: N = 70 (a partial second wavefront), T = 25 with a start in the last row, two consecutive starts, columns without
a start after row 0 and trailing weights = 0; T = 1; N = 1.  Maps: 4x4 at 32 and at 20 units (padding), chain at 32 (29
states: a partial row block of the weight sums), 8x8 at 32 (three row blocks), 4x4 at 32 without the previous action.
4x4 at 64 units does not fit the LDS of a CU next to its tangent vector: the refusal case.
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
# map, hidden, N, T, include_action
CASES = [("4x4", 32, 70, 25, True), ("4x4", 20, 70, 25, True), ("chain", 32, 70, 25, True), ("8x8", 32, 70, 25, True),
         ("4x4", 32, 70, 25, False), ("4x4", 32, 70, 1, True), ("4x4", 32, 1, 25, True)]


def _policy(desc, hidden, seed=0, scale=0.1, **kw):
    """(GridWorldEnv, CategoricalGRUPolicy(bptt_kernels=True)) with every parameter -- h0 and the biases too -- moved off
    its initial value."""
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    env = GridWorldEnv(desc)
    np.random.seed(seed)
    kw.setdefault("bptt_kernels", True)
    pol = CategoricalGRUPolicy(env.spec, hidden_dim=hidden, **kw)
    theta = pol.get_param_values()
    pol.set_param_values(theta + scale * np.random.RandomState(seed + 1).randn(theta.size))
    return env, pol


def _planes(pol, N, T, seed=3, at_old=False, edit=None):
    """Synthetic planes in the order of npo_inputs: random state and action indices as one-hot planes.  ``at_old``:
    old == new (the point the Fisher matrix is taken at); else the old probabilities are the softmax of the current logits
    plus 0.3 randn: lr != 1, the KL of order 1e-2.  ``edit(start, w)`` changes the start mask and the weights in place
    (numpy, [T, N]) behind the columns made here; it draws nothing from the generator."""
    rng = np.random.RandomState(seed)
    dev = pol.flat_params.device
    S, A = pol.obs_dim, pol.action_dim
    eye = lambda n, idx: torch.as_tensor(np.eye(n, dtype=np.float32)[idx].transpose(2, 0, 1).copy(), device=dev)
    obs, act = eye(S, rng.randint(0, S, size=(T, N))), eye(A, rng.randint(0, A, size=(T, N)))
    adv = torch.as_tensor(rng.randn(T, N).astype(np.float32), device=dev)
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
        prob = pol.dist_info_planes(obs, act, start)["prob"]
    if at_old:
        old = prob.clone()
    else:
        noise = torch.as_tensor(rng.randn(A, T, N).astype(np.float32), device=dev)
        old = torch.softmax(torch.log(prob) + 0.3 * noise, dim=0)
    inv = 1.0 / w.double().sum().cpu()
    return (obs, act, adv, old.contiguous(), start, w, inv)


def _closures(pol):
    """algos/npo.py's recurrent categorical closures."""
    dist = pol.distribution

    def surr_loss(flat, obs, act, adv, old_prob, start, w, inv_count):
        new = pol.dist_info_planes(obs, act, start, flat)
        lr = dist.likelihood_ratio_sym(act, dict(prob=old_prob), new, axis=0)
        return -(lr * adv * w).sum() * inv_count.to(lr.dtype)

    def mean_kl(flat, obs, act, adv, old_prob, start, w, inv_count):
        kl = dist.kl_sym(dict(prob=old_prob), pol.dist_info_planes(obs, act, start, flat), axis=0)
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
    desc, hidden, N, T, inc = case
    _, pol = _policy(desc, hidden, state_include_action=inc)
    ops = pol.fused_ops()
    assert ops is not None, pol.why_no_kernel_layout()
    inputs = _planes(pol, N, T)
    assert ops.accepts(inputs)
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
@pytest.mark.parametrize("hidden", [32, 20])
def test_forward_sweep_reproduces_the_rollouts_probabilities(hidden):
    N, T, MPL = 70, 25, 11
    env, pol = _policy("4x4", hidden)
    ve = env.vec_env_executor(N, MPL, seed=5)
    assert ve.takes_rollout_of(pol)
    traj = ve.rollout(pol, T)
    assert int(traj.dones.sum()) > 0
    start = torch.ones_like(traj.dones, dtype=torch.bool)
    start[1:] = traj.dones[:-1].bool()
    adv = torch.randn(T, N, device=traj.device)
    w = torch.ones(T, N, device=traj.device)
    inputs = (traj.obs, traj.actions, adv, traj.means, start, w, torch.tensor(1.0 / (T * N), dtype=torch.float64))
    ops = pol.fused_ops()
    assert ops.accepts(inputs)
    assert torch.equal(ops.forward_probs(inputs), traj.means)
    assert torch.equal(ops.forward_probs(inputs, with_grad=True), traj.means)
    ops.release()
    loss, kl = ops.loss_and_kl(inputs)
    assert kl == 0.0 and np.isfinite(loss)          # the KL's two logarithms are one expression: 0 at equal inputs


# -- 2. sums and gradient ------------------------------------------------------------------------------------------------------
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
    assert flat.dtype == torch.float64 and flat.numel() == ops.n_flat and bool(torch.all(flat[:pol.hidden_dim] == 0))
    assert torch.equal(flat[idx], g[idx])


def test_a_sample_of_weight_zero_contributes_nothing():
    """Whatever its planes hold: NaN advantages and old probabilities under w = 0 leave every result's bits alone."""
    r = _case(CASES[0])
    ops, inputs = r["ops"], r["inputs"]
    obs, act, adv, old, start, w, inv = inputs
    dead = w == 0
    assert int(dead.sum()) > 0
    adv2, old2 = adv.clone(), old.clone()
    adv2[dead] = float("nan")
    old2[:, dead] = float("nan")
    other = (obs, act, adv2, old2, start, w, inv)
    ops.release()
    g1 = ops.loss_grad_kernel(inputs, with_loss=True).clone()
    s1 = ops.loss_and_kl(inputs)
    ops.release()
    g2 = ops.loss_grad_kernel(other, with_loss=True).clone()
    s2 = ops.loss_and_kl(other)
    ops.release()
    assert s1 == s2 and torch.equal(g1, g2)


# -- 3. Fisher-vector product ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_fisher_vector_product_against_perlmutter(case):
    r = _case(case)
    pol, ops, idx = r["pol"], r["ops"], r["idx"]
    desc, hidden, N, T, inc = case
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


# -- 4. determinism ------------------------------------------------------------------------------------------------------------
def test_every_pass_twice_gives_the_same_bits():
    r = _case(CASES[2])                                  # chain: two row blocks of the weight sums, the second partial
    ops, inputs = r["ops"], r["inputs"]
    n = ops.n_kernel
    v = torch.as_tensor(np.random.RandomState(2).randn(n).astype(np.float32), device=inputs[0].device)
    v = ops.scatter(ops.gather(v))
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


# -- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_a_shape_over_the_lds_budget_launches_nothing():
    from rllab_amd import _lib
    lib = _lib.lib
    N, T, H, S = 8, 3, 64, 16
    dev = torch.device("cuda", 0)
    full = lambda *shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=dev)
    assert lib.rl_gru_categorical_workspace_bytes(N, T, S, H, 1) == 0
    msg = lib.rl_last_error().decode()
    assert "bytes of LDS" in msg and int(msg.split(":")[1].split()[0]) > 160 * 1024
    out2, grad, ws, prob = full(2, dtype=torch.float64), full(32768), full(1 << 20), full(4, T, N)
    planes = dict(theta=full(32768), state=full(T, N, dtype=torch.int32), action=full(T, N, dtype=torch.int32),
                  advantages=full(T, N), old_prob=full(4, T, N), start=full(T, N, dtype=torch.uint8), weights=full(T, N))
    b = _lib.GruCategoricalBatch(n_envs=N, horizon=T, n_states=S, n_act=4, hidden=H, include_action=1, inv_count=1.0,
                                 prob=prob.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 4,
                                 **{k: t.data_ptr() for k, t in planes.items()})
    assert lib.rl_gru_categorical_eval(ctypes.byref(b), out2.data_ptr(), None) == -2
    assert "bytes of LDS" in lib.rl_last_error().decode()
    assert lib.rl_gru_categorical_grad(ctypes.byref(b), out2.data_ptr(), grad.data_ptr(), None) == -2
    assert lib.rl_gru_categorical_fvp(ctypes.byref(b), planes["theta"].data_ptr(), grad.data_ptr(), None) == -2
    torch.cuda.synchronize()
    for name, t in dict(out2=out2, grad=grad, ws=ws, prob=prob).items():
        assert bool(torch.all(t == 7)), name                                   # nothing was launched
    # the policy says so and its update runs through autograd
    _, pol = _policy("4x4", 64)
    assert pol.fused_ops() is None and "bytes of LDS" in pol.why_no_kernel_layout()
    _, pol = _policy("4x4", 33)
    assert pol.kernel_hidden == 64 and pol.fused_ops() is None and "bytes of LDS" in pol.why_no_kernel_layout()


@pytest.mark.parametrize("case,sentence", [
    ("hidden", "hidden_dim=100: the recurrent update kernels run 1 .. 64 hidden units"),
    ("rectify", "hidden_nonlinearity is rectify (the recurrent update kernels evaluate tanh)")])
def test_policies_the_kernels_do_not_take_fall_back_to_autograd(case, sentence, tmp_path):
    from rllab_amd.algos.trpo import TRPO
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.core.network import rectify
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import logger
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    env = GridWorldEnv()
    kw = dict(hidden=dict(hidden_dim=100), rectify=dict(hidden_nonlinearity=rectify))[case]
    policy = CategoricalGRUPolicy(env_spec=env.spec, bptt_kernels=True, **kw)
    assert policy.fused_ops() is None and policy.why_no_kernel_layout() == sentence
    # (the fused rollout does not take these policies either: the update path is decided, and logged, by init_opt)
    algo = TRPO(env=env, policy=policy, baseline=ZeroBaseline(env_spec=env.spec), batch_size=200, max_path_length=20, n_itr=1)
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


# -- 6. end to end -----------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name", ["TRPO", "TNPG", "TRPO-fd", "VPG", "PPO"])
def test_algorithms_on_gridworld_with_the_recurrent_kernels(name, tmp_path):
    from rllab_amd.envs.grid_world_env import GridWorldEnv
    from rllab_amd.misc import ext
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    # TNPG takes the full natural-gradient step once and the optimizer rejects it when its KL exceeds step_size = 0.01,
    # which is where the quadratic model puts it.  The float32 AUTOGRAD update (bptt_kernels=False) of this very
    # configuration rejects the step at seeds 1, 5, 6 (theta does not move) and accepts it at seeds 2, 3, 4 with
    # MeanKL 0.00988, 0.00986, 0.00969; seed 4 has the widest margin, four orders of magnitude above what the two update
    # paths differ by.
    ext.set_seed(4 if name == "TNPG" else 1)
    env = GridWorldEnv()
    policy = CategoricalGRUPolicy(env_spec=env.spec, bptt_kernels=True)
    theta0 = policy.get_param_values()
    if name == "TRPO-fd":
        from rllab_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer, FiniteDifferenceHvp
        algo = _algo("TRPO", env, policy, optimizer_args=None,
                     optimizer=ConjugateGradientOptimizer(cg_iters=1, hvp_approach=FiniteDifferenceHvp(base_eps=1e-5)))
    else:
        algo = _algo(name, env, policy)
    text, rows = _train_logged(algo, tmp_path)
    theta = policy.get_param_values()
    assert "sampling path: fused rollout kernel" in text and len(rows) == 1
    if name in ("VPG", "PPO"):
        assert ("update path: torch autograd -- the recurrent kernels serve ConjugateGradientOptimizer (TRPO, TNPG)"
                in text)
        return
    assert "update path: HIP kernels (FusedCategoricalGRUOps)" in text
    assert "update path: torch autograd" not in text
    print(name, "MeanKLBefore", rows[0]["MeanKLBefore"], "MeanKL", rows[0]["MeanKL"], "dLoss", rows[0]["dLoss"])
    assert float(rows[0]["MeanKLBefore"]) == 0.0
    assert np.array_equal(theta[:32], theta0[:32])                       # h0 is not trainable
    assert np.all(np.isfinite(theta)) and np.abs(theta - theta0).max() > 0


# -- 7. learning ---------------------------------------------------------------------------------------------------------------------
def test_trpo_learns_gridworld_on_the_recurrent_kernels(tmp_path):
    """examples/trpo_gridworld_gru.py's configuration with --bptt-kernels (the optimizer's default products: the
    Fisher-vector kernel), seed 1, against the criteria of test_gpu_categorical_gru.py's learning test and its committed
    CPU yardstick: every iteration MeanKL <= 0.0101, LossAfter < LossBefore and MeanKLBefore == 0.0; the mean return of
    the last three iterations exceeds that of the first three by at least half the yardstick's gain."""
    from examples.trpo_gridworld_gru import CONFIG, make_algo
    with open(os.path.join(ROOT, "profiles", "curves", "trpo_gridworld_gru_cpu.csv")) as f:
        cpu = [float(r["AverageReturn"]) for r in csv.DictReader(f)]
    assert len(cpu) == CONFIG["n_itr"]
    cpu_gain = np.mean(cpu[-3:]) - np.mean(cpu[:3])
    assert cpu_gain >= 0.2, cpu
    text, rows = _train_logged(make_algo(seed=1, bptt_kernels=True), tmp_path)
    assert "update path: HIP kernels (FusedCategoricalGRUOps)" in text and len(rows) == CONFIG["n_itr"]
    ret = [float(r["AverageReturn"]) for r in rows]
    print("AverageReturn", ret, "CPU", cpu)
    for r in rows:
        print(r["Iteration"], r["LossBefore"], r["LossAfter"], r["MeanKLBefore"], r["MeanKL"])
    for r in rows:
        assert float(r["MeanKLBefore"]) == 0.0, r
        assert float(r["MeanKL"]) <= 0.0101, r
        assert float(r["LossAfter"]) < float(r["LossBefore"]), r
    assert np.mean(ret[-3:]) - np.mean(ret[:3]) >= 0.5 * cpu_gain, (ret, cpu_gain)
