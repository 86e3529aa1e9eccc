"""GaussianGRUPolicy on the host (no GPU): parameter layout, the forward pass over planes against an independent numpy
restatement of the step function, zero padding to the kernel's widths, the autograd gradient, pickling and the alias.
The reference's own files are rllab/policies/gaussian_gru_policy.py and rllab/core/network.py:104-270."""
import ast
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

REF_EXAMPLE = "/root/reference/examples/trpo_cartpole_recurrent.py"
ORDER = ["h0", "W_xr", "W_hr", "b_r", "W_xu", "W_hu", "b_u", "W_xc", "W_hc", "b_c", "output.W", "output.b",
         "output_log_std.param"]


def _spec(do, da):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Box
    return EnvSpec(Box(-np.ones(do), np.ones(do)), Box(-np.ones(da), np.ones(da)))


def _policy(do=4, da=1, hidden=32, seed=0, randomize=True, **kw):
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    np.random.seed(seed)
    pol = GaussianGRUPolicy(_spec(do, da), hidden_sizes=(hidden,), **kw)
    if randomize:       # biases, h0 and log_std away from their initial zeros, so that every term of the step matters
        theta = pol.get_param_values()
        pol.set_param_values(theta + 0.3 * np.random.RandomState(seed + 1).randn(theta.size))
    return pol


def _shapes(do, da, H, include_action):
    di = do + (da if include_action else 0)
    return [(H,), (di, H), (H, H), (H,), (di, H), (H, H), (H,), (di, H), (H, H), (H,), (H, da), (da,), (da,)]


# -- parameters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_action", [True, False])
def test_parameter_count_and_order(include_action):
    do, da, H = 4, 1, 32
    pol = _policy(do, da, H, randomize=False, state_include_action=include_action, init_std=0.5)
    shapes = _shapes(do, da, H, include_action)
    theta = pol.get_param_values()
    assert theta.size == sum(int(np.prod(s)) for s in shapes)
    assert [p.name for p in pol.get_params()] == ORDER
    assert pol.get_param_shapes() == shapes
    off = 0
    for name, shape in zip(ORDER, shapes):
        size = int(np.prod(shape))
        block = theta[off:off + size].reshape(shape)
        off += size
        assert np.array_equal(block, pol._by_name[name].get_value().astype(np.float64)), name
        if len(shape) == 2:            # Glorot-uniform: inside the bound, and not degenerate
            bound = np.sqrt(6.0 / (shape[0] + shape[1]))
            assert np.abs(block).max() <= bound + 1e-7 and block.std() > 0.3 * bound, name
        elif name == "output_log_std.param":
            assert np.allclose(block, np.log(0.5), atol=1e-7)
        else:
            assert np.all(block == 0), name
    # writing one named matrix moves exactly its slice
    marked = np.zeros_like(theta)
    w_hu = ORDER.index("W_hu")
    a = sum(int(np.prod(s)) for s in shapes[:w_hu])
    marked[a:a + H * H] = np.arange(H * H)
    pol.set_param_values(marked)
    assert np.array_equal(pol._by_name["W_hu"].get_value(), np.arange(H * H, dtype=np.float32).reshape(H, H))
    assert pol.recurrent and pol.vectorized
    assert pol.state_info_keys == (["prev_action"] if include_action else [])


def test_trainable_and_regularizable_sets():
    do, da, H = 4, 1, 32
    pol = _policy(do, da, H)
    names = lambda **tags: [p.name for p in pol.get_params(**tags)]
    assert names(trainable=True) == ORDER[1:]
    assert pol.get_param_values(trainable=True).size == pol.get_param_values().size - H
    assert names(regularizable=True) == ["W_xr", "W_hr", "W_xu", "W_hu", "W_xc", "W_hc", "output.W", "output_log_std.param"]
    fixed = _policy(do, da, H, learn_std=False)
    assert [p.name for p in fixed.get_params(trainable=True)] == ORDER[1:-1]
    assert fixed.get_param_values(trainable=True).size == fixed.get_param_values().size - H - da
    # set_param_values(trainable=True) leaves h0 (and the fixed log_std) alone
    before = fixed.get_param_values()
    fixed.set_param_values(np.zeros(before.size - H - da), trainable=True)
    after = fixed.get_param_values()
    assert np.array_equal(after[:H], before[:H]) and np.array_equal(after[-da:], before[-da:])
    assert np.all(after[H:-da] == 0)
    with pytest.raises(AssertionError):
        from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
        GaussianGRUPolicy(_spec(4, 1), hidden_sizes=(32, 32))


# -- the definition against a numpy restatement ---------------------------------------------------------------------------
def _np_step(p, x, h):
    """The step function, from the formulas of rllab/core/network.py:150-155, numpy float64."""
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    r = sig(x @ p["W_xr"] + h @ p["W_hr"] + p["b_r"])
    u = sig(x @ p["W_xu"] + h @ p["W_hu"] + p["b_u"])
    c = np.tanh(x @ p["W_xc"] + r * (h @ p["W_hc"]) + p["b_c"])
    h = (1 - u) * h + u * c
    return h, h @ p["output.W"] + p["output.b"]


def _named(pol, shapes):
    theta, out, off = pol.get_param_values(), {}, 0
    for name, shape in zip(ORDER, shapes):
        size = int(np.prod(shape))
        out[name] = theta[off:off + size].reshape(shape)
        off += size
    return out


def _batch(do, da, T=25, N=7, seed=3):
    """Planes with path ends at irregular places: a path of one step at t = 0 (so another starts at t = 1), one that starts
    at t = T - 1, columns without any end."""
    rng = np.random.RandomState(seed)
    obs = rng.randn(do, T, N)
    act = rng.randn(da, T, N)
    done = np.zeros((T, N), dtype=bool)
    done[0, 1] = True
    done[T - 2, 2] = True
    done[[3, 4, 11], 3] = True
    done[[7, 19], 4] = True
    done[T - 1, 5] = True
    done[[9, T - 2, T - 1], 6] = True
    start = np.ones((T, N), dtype=bool)
    start[1:] = done[:-1]
    return obs, act, done, start


@pytest.mark.parametrize("include_action", [True, False])
@pytest.mark.parametrize("do,da,H", [(4, 1, 32), (13, 2, 20)])
def test_dist_info_planes_equals_numpy_restatement(do, da, H, include_action):
    pol = _policy(do, da, H, state_include_action=include_action)
    p = _named(pol, _shapes(do, da, H, include_action))
    obs, act, done, start = _batch(do, da)
    T, N = done.shape
    assert start[0].all() and start[T - 1, 2] and start[1, 1]
    want = np.zeros((da, T, N))
    for n in range(N):                                    # path by path, stepping like get_action
        h, prev = None, None
        for t in range(T):
            if start[t, n]:
                h, prev = p["h0"].copy(), np.zeros(da)
            x = np.concatenate([obs[:, t, n], prev]) if include_action else obs[:, t, n]
            h, mean = _np_step(p, x, h)
            want[:, t, n] = mean
            prev = act[:, t, n]
    flat64 = torch.as_tensor(pol.get_param_values(), dtype=torch.float64, device=pol.flat_params.device)
    dev = flat64.device
    with torch.no_grad():
        got = pol.dist_info_planes(torch.as_tensor(obs, device=dev), torch.as_tensor(act, device=dev),
                                   torch.as_tensor(start, device=dev), flat64)
    assert got["mean"].dtype == torch.float64 and tuple(got["mean"].shape) == (da, T, N)
    err = np.abs(got["mean"].cpu().numpy() - want).max()
    print("dist_info_planes vs numpy restatement (%d, %d, %d): max |diff| = %.3e" % (do, da, H, err))
    assert err <= 1e-12
    assert np.array_equal(got["log_std"].reshape(-1).cpu().numpy(), p["output_log_std.param"])


def test_host_stepping_follows_the_definition():
    """reset / get_action / get_actions (numpy in, numpy out): the means they report are those of dist_info_planes on the
    observations and the actions THEY sampled, prev_action is the previous sampled action, zeros after a reset."""
    do, da, H = 4, 1, 32
    pol = _policy(do, da, H)
    rng = np.random.RandomState(5)
    np.random.seed(11)
    T = 9
    obs = rng.randn(T, do)
    pol.reset()
    acts, means, prevs = [], [], []
    for t in range(T):
        if t == 4:
            pol.reset()
        a, info = pol.get_action(obs[t])
        assert a.shape == (da,) and set(info) == {"mean", "log_std", "prev_action"}
        acts.append(a); means.append(info["mean"]); prevs.append(info["prev_action"])
    acts, means, prevs = np.array(acts), np.array(means), np.array(prevs)
    assert np.all(prevs[0] == 0) and np.all(prevs[4] == 0)
    assert np.array_equal(prevs[1:4], acts[0:3]) and np.array_equal(prevs[5:], acts[4:-1])
    start = np.zeros((T, 1), dtype=bool)
    start[[0, 4]] = True
    dev = pol.flat_params.device
    flat64 = torch.as_tensor(pol.get_param_values(), dtype=torch.float64, device=dev)
    with torch.no_grad():
        d = pol.dist_info_planes(torch.as_tensor(obs.T[:, :, None].copy(), device=dev),
                                 torch.as_tensor(acts.T[:, :, None].copy(), device=dev),
                                 torch.as_tensor(start, device=dev), flat64)
    assert np.abs(d["mean"][:, :, 0].t().cpu().numpy() - means).max() <= 1e-12
    # the vectorised form: reset(dones) puts back the rows that are done and no others
    pol.reset(dones=[True, True, True])
    o3 = rng.randn(3, do)
    a1, i1 = pol.get_actions(o3)
    assert a1.shape == (3, da) and np.all(i1["prev_action"] == 0)
    pol.reset(dones=[False, True, False])
    a2, i2 = pol.get_actions(o3)
    assert np.array_equal(i2["prev_action"][[0, 2]], a1[[0, 2]]) and np.all(i2["prev_action"][1] == 0)
    assert np.array_equal(i2["mean"][1], i1["mean"][1]) and not np.array_equal(i2["mean"][0], i1["mean"][0])
    # dist_info_sym, the reference-shaped wrapper ([N, T, .] in and out)
    sym = pol.dist_info_sym(obs[None, :4], dict(prev_action=prevs[None, :4]))
    assert tuple(sym["mean"].shape) == (1, 4, da) and tuple(sym["log_std"].shape) == (1, 4, da)
    assert np.abs(sym["mean"][0].detach().cpu().numpy() - means[:4]).max() <= 1e-5        # (float32 parameters)


# -- zero padding to the kernel's widths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_action", [True, False])
def test_zero_padded_layout_gives_the_same_means(include_action):
    do, da, H = 13, 2, 20
    pol = _policy(do, da, H, state_include_action=include_action)
    assert pol.kernel_hidden == 32 and _policy(do, da, 33, randomize=False).kernel_hidden == 64
    idx, size = pol.pad_index()
    wide = _policy(do, da, 32, randomize=False, state_include_action=include_action)
    assert size == wide.get_param_values().size and np.unique(idx).size == idx.size == pol.get_param_values().size
    padded = np.zeros(size)
    padded[idx] = pol.get_param_values()
    wide.set_param_values(padded)
    # every named block of the padded vector is the narrow one in its top-left corner, zeros elsewhere
    for name in ORDER:
        small, big = pol._by_name[name].get_value(), wide._by_name[name].get_value()
        corner = tuple(slice(0, s) for s in small.shape)
        assert np.array_equal(big[corner], small), name
        assert np.count_nonzero(big) == np.count_nonzero(small), name
    obs, act, done, start = _batch(do, da)
    dev = pol.flat_params.device
    args = (torch.as_tensor(obs, device=dev), torch.as_tensor(act, device=dev), torch.as_tensor(start, device=dev))
    with torch.no_grad():
        a = pol.dist_info_planes(*args, pol.flat_params.double())["mean"]
        b = wide.dist_info_planes(*args, wide.flat_params.double())["mean"]
    assert torch.equal(a, b)
    if not pol.flat_params.is_cuda:
        assert pol.rollout_layout() is None and "HIP device" in pol.why_no_rollout_kernel()


def test_shape_limits_are_said_in_a_sentence():
    from rllab_amd.core.network import rectify
    assert "hidden_sizes=(100,)" in _policy(4, 1, 100, randomize=False).why_no_rollout_kernel()
    assert "rectify" in _policy(4, 1, 32, randomize=False, hidden_nonlinearity=rectify).why_no_rollout_kernel()
    assert "output_nonlinearity" in _policy(4, 1, 32, randomize=False, output_nonlinearity=torch.tanh).why_no_rollout_kernel()
    assert "obs_dim 31" in _policy(31, 1, 32, randomize=False).why_no_rollout_kernel()
    assert "action_dim 9" in _policy(4, 9, 32, randomize=False).why_no_rollout_kernel()


# -- gradient -------------------------------------------------------------------------------------------------------------
def test_vpg_objective_gradient_matches_finite_differences():
    do, da, H = 4, 1, 8
    pol = _policy(do, da, H)
    obs, act, done, start = _batch(do, da)
    rng = np.random.RandomState(9)
    adv = rng.randn(*done.shape)
    valid = np.ones(done.shape)
    valid[20:, 0] = 0                                       # a trailing unfinished path
    dev = pol.flat_params.device
    t = lambda x: torch.as_tensor(x, device=dev)
    obs_t, act_t, start_t, adv_t, w_t = t(obs), t(act), t(start), t(adv), t(valid)
    dist = pol.distribution

    def objective(flat):
        logli = dist.log_likelihood_sym(act_t, pol.dist_info_planes(obs_t, act_t, start_t, flat), axis=0)
        return -(logli * adv_t * w_t).sum() / w_t.sum()

    theta = torch.as_tensor(pol.get_param_values(), dtype=torch.float64, device=dev)
    flat = theta.clone().requires_grad_(True)
    grad = torch.autograd.grad(objective(flat), flat)[0].cpu().numpy()
    fd = np.zeros_like(grad)
    eps = 1e-6
    with torch.no_grad():
        for i in range(theta.numel()):
            e = torch.zeros_like(theta)
            e[i] = eps
            fd[i] = float(objective(theta + e) - objective(theta - e)) / (2 * eps)
    rel = np.abs(grad - fd).max() / np.abs(fd).max()
    print("VPG objective: autograd vs central differences, relative %.3e (|grad|max %.3e)" % (rel, np.abs(fd).max()))
    assert rel <= 1e-6
    assert np.abs(grad[:H]).max() > 0          # h0 has a gradient; it is the optimizers' trainable index that leaves it alone


# -- pickle, alias ----------------------------------------------------------------------------------------------------------
def test_pickle_round_trip_keeps_the_parameters():
    pol = _policy(4, 1, 20, state_include_action=False, learn_std=False, init_std=0.7)
    clone = pickle.loads(pickle.dumps(pol))
    assert np.array_equal(clone.get_param_values(), pol.get_param_values())
    assert clone.hidden_dim == 20 and clone.state_info_keys == [] and not clone.learn_std
    assert [p.name for p in clone.get_params(trainable=True)] == ORDER[1:-1]
    v0 = pol.param_version()
    pol.set_param_values(pol.get_param_values() * 0.5)
    assert pol.param_version() != v0


def test_alias_imports_resolve():
    from rllab.distributions.recurrent_diagonal_gaussian import RecurrentDiagonalGaussian
    from rllab.distributions.diagonal_gaussian import DiagonalGaussian
    from rllab.policies.gaussian_gru_policy import GaussianGRUPolicy
    import rllab_amd.policies.gaussian_gru_policy as mod
    assert GaussianGRUPolicy is mod.GaussianGRUPolicy and RecurrentDiagonalGaussian is DiagonalGaussian
    assert isinstance(_policy().distribution, RecurrentDiagonalGaussian)


@pytest.mark.skipif(not os.path.isfile(REF_EXAMPLE), reason="reference tree not mounted")
def test_reference_recurrent_example_binds_to_our_api():
    tree = ast.parse(open(REF_EXAMPLE).read())
    imported = 0
    for node in tree.body:
        if isinstance(node, ast.ImportFrom):
            mod = importlib.import_module(node.module)       # rllab.* alias -> rllab_amd.*
            assert mod.__name__.startswith("rllab_amd."), mod.__name__
            for a in node.names:
                assert hasattr(mod, a.name), (node.module, a.name)
                imported += 1
    assert imported >= 7


def test_finite_difference_hvp_of_a_gru_policy_is_evaluated_in_float64():
    """FiniteDifferenceHvp(base_eps=1e-5) shifts the parameters by about 1e-6: the two shifted gradients of a GRU policy
    are evaluated in float64 (``fd_hvp_dtype``), so the product agrees with double back-propagation in float64 at the
    same float32 parameters.  Central differences in float64: truncation ~ eps^2, rounding ~ 1e-16 / eps = 1e-10 of
    the gradient's size; the bound 1e-5 leaves four orders of magnitude."""
    from rllab_amd.optimizers.conjugate_gradient_optimizer import FiniteDifferenceHvp
    do, da, H = 4, 1, 32
    pol = _policy(do, da, H)
    assert pol.flat_params.dtype == torch.float32 and pol.fd_hvp_dtype == torch.float64
    obs, act, done, start = _batch(do, da)
    dev = pol.flat_params.device
    t32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)
    obs_t, act_t, start_t = t32(obs), t32(act), torch.as_tensor(start, device=dev)
    dist = pol.distribution
    with torch.no_grad():
        old = pol.dist_info_planes(obs_t, act_t, start_t)
    old = dict(mean=old["mean"] + 0.05, log_std=old["log_std"] - 0.02)          # away from the minimum of the KL

    def mean_kl(flat, *inputs):
        return dist.kl_sym(old, pol.dist_info_planes(obs_t, act_t, start_t, flat), axis=0).mean()

    idx = pol._flat_index(trainable=True)
    hvp = FiniteDifferenceHvp(base_eps=1e-5)
    hvp.update_opt(f=mean_kl, target=pol, inputs=None, reg_coeff=0.0)
    x = torch.as_tensor(np.random.RandomState(2).randn(idx.numel()), dtype=torch.float64, device=dev)
    got = hvp.build_eval((), idx)(x)
    flat = pol.flat_params.detach().double().requires_grad_(True)
    g = torch.autograd.grad(mean_kl(flat), flat, create_graph=True)[0]
    xf = torch.zeros_like(flat)
    xf[idx] = x
    want = torch.autograd.grad((g * xf).sum(), flat)[0][idx]
    rel = float((got - want).abs().max() / want.abs().max())
    print("FiniteDifferenceHvp vs double back-propagation: relative %.3e" % rel)
    assert got.dtype == torch.float64 and rel <= 1e-5
