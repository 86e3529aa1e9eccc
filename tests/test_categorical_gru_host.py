"""CategoricalGRUPolicy and RecurrentCategorical on the host (no GPU): parameter layout, the forward pass over planes against
an independent numpy restatement of the step function and the softmax, zero padding to the kernel's widths, the autograd
gradient, the distribution's formulas, host stepping, pickling, the aliases and the ABI mirror of the rollout's struct.
The reference's own files are rllab/policies/categorical_gru_policy.py, rllab/distributions/recurrent_categorical.py and
rllab/core/network.py:104-270."""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ["h0", "W_xr", "W_hr", "b_r", "W_xu", "W_hu", "b_u", "W_xc", "W_hc", "b_c", "output.W", "output.b"]
TINY = 1e-8


def _spec(S, A):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Discrete
    return EnvSpec(Discrete(S), Discrete(A))


def _policy(S=16, A=4, hidden=32, seed=0, randomize=True, **kw):
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    np.random.seed(seed)
    pol = CategoricalGRUPolicy(_spec(S, A), hidden_dim=hidden, **kw)
    if randomize:       # biases and h0 away from their initial zeros, so that every term of the step matters
        theta = pol.get_param_values()
        pol.set_param_values(theta + 0.3 * np.random.RandomState(seed + 1).randn(theta.size))
    return pol


def _shapes(S, A, H, include_action):
    di = S + (A if include_action else 0)
    return [(H,), (di, H), (H, H), (H,), (di, H), (H, H), (H,), (di, H), (H, H), (H,), (H, A), (A,)]


def _named(pol, shapes):
    theta, out, off = pol.get_param_values(), {}, 0
    for name, shape in zip(ORDER, shapes):
        size = int(np.prod(shape))
        out[name] = theta[off:off + size].reshape(shape)
        off += size
    assert off == theta.size
    return out


def _batch(S, A, T=12, N=5, seed=3):
    """One-hot planes with path starts inside them: a path of one step at t = 0 (so another starts at t = 1), one that
    starts at t = T - 1, a column without any end."""
    rng = np.random.RandomState(seed)
    obs = np.eye(S)[rng.randint(0, S, size=(T, N))].transpose(2, 0, 1).copy()
    act = np.eye(A)[rng.randint(0, A, size=(T, N))].transpose(2, 0, 1).copy()
    done = np.zeros((T, N), dtype=bool)
    done[0, 1] = True
    done[T - 2, 2] = True
    done[[3, 4, 8], 3] = True
    done[[5, T - 2, T - 1], 4] = True
    start = np.ones((T, N), dtype=bool)
    start[1:] = done[:-1]
    return obs, act, done, start


def _planes(pol, obs, act, start, flat):
    dev = flat.device
    with torch.no_grad():
        return pol.dist_info_planes(torch.as_tensor(obs, device=dev), torch.as_tensor(act, device=dev),
                                    torch.as_tensor(start, device=dev), flat)["prob"]


def _flat64(pol):
    return torch.as_tensor(pol.get_param_values(), dtype=torch.float64, device=pol.flat_params.device)


# -- parameters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_action", [True, False])
def test_parameter_count_order_and_initial_values(include_action):
    S, A, H = 16, 4, 32
    pol = _policy(S, A, H, randomize=False, state_include_action=include_action)
    shapes = _shapes(S, A, H, include_action)
    theta = pol.get_param_values()
    assert theta.size == sum(int(np.prod(s)) for s in shapes)
    assert [p.name for p in pol.get_params()] == ORDER
    assert pol.get_param_shapes() == shapes
    assert pol.flat_params.dtype == torch.float32 and pol.flat_params.dim() == 1
    for name, block in _named(pol, shapes).items():
        if block.ndim == 2:            # Glorot-uniform: inside the bound, and not degenerate
            bound = np.sqrt(6.0 / (block.shape[0] + block.shape[1]))
            assert np.abs(block).max() <= bound + 1e-7 and block.std() > 0.3 * bound, name
        else:                          # zero biases and h0
            assert np.all(block == 0), name
    assert [p.name for p in pol.get_params(trainable=True)] == ORDER[1:]             # h0 is not trainable
    assert pol.get_param_values(trainable=True).size == theta.size - H
    before = _policy(S, A, H, state_include_action=include_action)
    h0 = before.get_param_values()[:H].copy()
    before.set_param_values(np.zeros(theta.size - H), trainable=True)
    assert np.array_equal(before.get_param_values()[:H], h0) and np.all(before.get_param_values()[H:] == 0)
    assert pol.recurrent and pol.vectorized and pol.state_include_action == include_action
    assert pol.state_info_keys == (["prev_action"] if include_action else [])
    assert pol.distribution.dist_info_keys == ["prob"] and pol.distribution.dim == A


def test_gaussian_gru_specs_are_what_they_were():
    """``gru_param_specs`` drops the log-std row only when asked to."""
    from rllab_amd.policies.gaussian_gru_policy import gru_param_specs
    full = gru_param_specs(5, 32, 2)
    assert [s[0] for s in full] == ORDER + ["output_log_std.param"] and full[-1] == ("output_log_std.param", (2,), True, True)
    assert gru_param_specs(5, 32, 2, learn_std=False)[-1][2] is False
    assert gru_param_specs(5, 32, 2, log_std_row=False) == full[:-1]


# -- the definition against a numpy restatement ---------------------------------------------------------------------------
def _np_step(p, x, h):
    """The step function from the formulas of rllab/core/network.py:150-155 and a max-subtracted softmax, numpy float64."""
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    r = sig(x @ p["W_xr"] + h @ p["W_hr"] + p["b_r"])
    u = sig(x @ p["W_xu"] + h @ p["W_hu"] + p["b_u"])
    c = np.tanh(x @ p["W_xc"] + r * (h @ p["W_hc"]) + p["b_c"])
    h = (1 - u) * h + u * c
    z = h @ p["output.W"] + p["output.b"]
    e = np.exp(z - z.max())
    return h, e / e.sum()


def _np_planes(p, obs, act, start, A, include_action):
    _, T, N = obs.shape
    want = np.zeros((A, T, N))
    for n in range(N):                                    # path by path, stepping like get_action
        h, prev = None, None
        for t in range(T):
            if start[t, n]:
                h, prev = p["h0"].copy(), np.zeros(A)
            x = np.concatenate([obs[:, t, n], prev]) if include_action else obs[:, t, n]
            h, prob = _np_step(p, x, h)
            want[:, t, n] = prob
            prev = act[:, t, n]
    return want


@pytest.mark.parametrize("include_action", [True, False])
def test_dist_info_planes_equals_numpy_restatement(include_action):
    S, A, H = 16, 4, 32
    pol = _policy(S, A, H, state_include_action=include_action)
    p = _named(pol, _shapes(S, A, H, include_action))
    obs, act, done, start = _batch(S, A)
    T, N = done.shape
    assert (T, N) == (12, 5) and start[0].all() and start[1, 1] and start[T - 1, 2] and not start[1:, 0].any()
    want = _np_planes(p, obs, act, start, A, include_action)
    got = _planes(pol, obs, act, start, _flat64(pol))
    assert got.dtype == torch.float64 and tuple(got.shape) == (A, T, N)
    err = np.abs(got.cpu().numpy() - want).max()
    print("dist_info_planes vs numpy restatement: max |diff| = %.3e" % err)
    assert err <= 1e-12
    assert np.abs(got.sum(dim=0).cpu().numpy() - 1).max() <= 1e-12
    if include_action:            # the previous action matters: other actions, other probabilities behind them
        other = _planes(pol, obs, np.roll(act, 1, axis=0), start, _flat64(pol))
        assert float((other - got).abs().max()) > 1e-3
        assert torch.equal(other[:, 0], got[:, 0])


# -- zero padding to the kernel's widths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_action", [True, False])
def test_zero_padded_layout_gives_the_same_probabilities(include_action):
    S, A, H = 16, 4, 20
    pol = _policy(S, A, H, state_include_action=include_action)
    assert pol.kernel_hidden == 32 and _policy(S, A, 33, randomize=False).kernel_hidden == 64
    assert _policy(S, A, 100, randomize=False).kernel_hidden is None
    idx, size = pol.pad_index()
    wide = _policy(S, A, 32, randomize=False, state_include_action=include_action)
    assert size == wide.get_param_values().size and np.unique(idx).size == idx.size == pol.get_param_values().size
    padded = np.zeros(size)
    padded[idx] = pol.get_param_values()
    wide.set_param_values(padded)
    # every named block of the padded vector is the narrow one in its top-left corner, zeros elsewhere
    small_p, wide_p = _named(pol, _shapes(S, A, H, include_action)), _named(wide, _shapes(S, A, 32, include_action))
    for name in ORDER:
        small, big = small_p[name], wide_p[name]
        corner = tuple(slice(0, s) for s in small.shape)
        assert np.array_equal(big[corner], small), name
        assert np.count_nonzero(big) == np.count_nonzero(small), name
    obs, act, done, start = _batch(S, A)
    a = _planes(pol, obs, act, start, pol.flat_params.double())
    b = _planes(wide, obs, act, start, wide.flat_params.double())
    assert torch.equal(a, b)
    # the padded units stay exactly 0: step the wide policy's planes by hand
    v = wide._views(wide.flat_params.double())
    dev = wide.flat_params.device
    h = v["h0"][:, None].expand(32, obs.shape[2])
    for t in range(4):
        x = torch.as_tensor(np.concatenate([obs[:, t], act[:, t]]) if include_action else obs[:, t], device=dev)
        with torch.no_grad():
            h, _ = wide.step_planes(x, h, v)
        assert bool((h[H:] == 0).all()) and float(h[:H].abs().min()) > 0
    if not pol.flat_params.is_cuda:
        assert pol.rollout_layout() is None and "HIP device" in pol.why_no_rollout_kernel()


def test_shape_limits_are_said_in_a_sentence():
    from rllab_amd.core.network import rectify
    assert "hidden_dim=100" in _policy(16, 4, 100, randomize=False).why_no_rollout_kernel()
    assert "rectify" in _policy(16, 4, 32, randomize=False, hidden_nonlinearity=rectify).why_no_rollout_kernel()
    # the LDS of a CU: 340 states fit at hidden 32 and 99 at hidden 64; 400 and 128 do not
    for S, H, fits in ((340, 32, True), (400, 32, False), (99, 64, True), (128, 64, False), (64, 64, True)):
        why = _policy(S, 4, H, randomize=False).why_no_rollout_kernel()
        assert ("bytes of LDS" in (why or "")) == (not fits), (S, H, why)
    assert _policy().why_no_kernel_layout() == "recurrent policy (no BPTT kernels)"


# -- dist_info_sym ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_action", [True, False])
def test_dist_info_sym_is_dist_info_planes_on_the_permuted_planes(include_action):
    S, A, H = 16, 4, 32
    pol = _policy(S, A, H, state_include_action=include_action)
    rng = np.random.RandomState(4)
    N, T = 3, 7
    obs = np.eye(S)[rng.randint(0, S, size=(N, T))]                       # [N, T, S]: one path per row
    acts = np.eye(A)[rng.randint(0, A, size=(N, T))]
    prev = np.concatenate([np.zeros((N, 1, A)), acts[:, :-1]], axis=1)
    sym = pol.dist_info_sym(obs, dict(prev_action=prev))["prob"]
    assert tuple(sym.shape) == (N, T, A)
    start = np.zeros((T, N), dtype=bool)
    start[0] = True
    # the same float32 arithmetic on differently strided operands: a matrix product may sum in another order, so a few
    # float32 ulps of a probability (<= 1), not bit equality
    want = _planes(pol, obs.transpose(2, 1, 0), acts.transpose(2, 1, 0), start, pol.flat_params)
    assert sym.dtype == torch.float32 and float((sym.detach() - want.permute(2, 1, 0)).abs().max()) <= 1e-6
    # and against the float64 definition, at float32 parameters
    want64 = _planes(pol, obs.transpose(2, 1, 0), acts.transpose(2, 1, 0), start, _flat64(pol))
    assert float((sym.detach().double() - want64.permute(2, 1, 0)).abs().max()) <= 1e-5


# -- gradient -------------------------------------------------------------------------------------------------------------
def test_masked_surrogate_gradient_matches_finite_differences():
    S, A, H = 6, 4, 8
    pol = _policy(S, A, H)
    obs, act, done, start = _batch(S, A)
    rng = np.random.RandomState(9)
    adv = rng.randn(*done.shape)
    valid = np.ones(done.shape)
    valid[9:, 0] = 0                                       # a trailing unfinished path
    dev = pol.flat_params.device
    t = lambda x: torch.as_tensor(x, device=dev)
    obs_t, act_t, start_t, adv_t, w_t = t(obs), t(act), t(start), t(adv), t(valid)
    dist = pol.distribution
    theta = _flat64(pol)
    old = dict(prob=torch.softmax(t(rng.randn(A, *done.shape)), dim=0))

    def objective(flat):
        lr = dist.likelihood_ratio_sym(act_t, old, pol.dist_info_planes(obs_t, act_t, start_t, flat), axis=0)
        return -(lr * adv_t * w_t).sum() / w_t.sum()

    flat = theta.clone().requires_grad_(True)
    g = torch.autograd.grad(objective(flat), flat, create_graph=True)[0]
    grad = g.detach().cpu().numpy()
    fd = np.zeros_like(grad)
    eps = 1e-6
    with torch.no_grad():
        for i in range(theta.numel()):
            e = torch.zeros_like(theta)
            e[i] = eps
            fd[i] = float(objective(theta + e) - objective(theta - e)) / (2 * eps)
    rel = np.abs(grad - fd).max() / np.abs(fd).max()
    print("masked surrogate: autograd vs central differences, relative %.3e (|grad|max %.3e)" % (rel, np.abs(fd).max()))
    assert rel <= 1e-6
    assert np.abs(grad[:H]).max() > 0          # h0 has a gradient; it is the optimizers' trainable index that leaves it alone
    # differentiable twice (PerlmutterHvp): a Hessian-vector product exists and is not identically zero
    hv = torch.autograd.grad((g * torch.ones_like(g)).sum(), flat)[0]
    assert bool(torch.isfinite(hv).all()) and float(hv.abs().max()) > 0


# -- RecurrentCategorical -----------------------------------------------------------------------------------------------------
def test_recurrent_categorical_formulas():
    """The reference's definitions (rllab/distributions/recurrent_categorical.py:19-71, categorical.py:32-73), transcribed in
    numpy on [N, T, 4] probabilities; the ``*_sym`` twins on the same layout and on the engine's [4, T, N] planes."""
    from rllab_amd.distributions.categorical import Categorical
    from rllab_amd.distributions.recurrent_categorical import RecurrentCategorical
    rng = np.random.RandomState(0)
    N, T, A = 5, 7, 4
    soft = lambda z: np.exp(z) / np.exp(z).sum(axis=-1, keepdims=True)
    old, new = soft(rng.randn(N, T, A)), soft(rng.randn(N, T, A))
    idx = rng.randint(0, A, size=(N, T))
    xs = np.eye(A)[idx]
    dist = RecurrentCategorical(A)
    assert isinstance(dist, Categorical) and dist.dim == A and dist.dist_info_keys == ["prob"]
    kl = np.sum(old * (np.log(old + TINY) - np.log(new + TINY)), axis=2)
    ent = -np.sum(new * np.log(new + TINY), axis=2)
    pick = lambda p: np.take_along_axis(p, idx[..., None], axis=2)[..., 0]
    logli = np.log(pick(new) + TINY)
    lr = (pick(new) + TINY) / (pick(old) + TINY)
    assert np.abs(dist.kl(dict(prob=old), dict(prob=new)) - kl).max() <= 1e-15
    assert np.abs(dist.entropy(dict(prob=new)) - ent).max() <= 1e-15
    got = dist.log_likelihood(xs, dict(prob=new))
    assert got.shape == (N, T) and np.abs(got - logli).max() <= 1e-15
    assert np.abs(dist.log_likelihood(xs[0], dict(prob=new[0])) - logli[0]).max() <= 1e-15     # [B, A] as Categorical's
    t = torch.as_tensor
    for axis, perm in ((-1, (0, 1, 2)), (0, (2, 1, 0))):         # [N, T, A], and planes [A, T, N]
        o, n_, x = (t(np.ascontiguousarray(a.transpose(perm))) for a in (old, new, xs))
        back = (lambda r: r.numpy()) if axis == -1 else (lambda r: r.numpy().T)
        assert np.abs(back(dist.kl_sym(dict(prob=o), dict(prob=n_), axis=axis)) - kl).max() <= 1e-15
        assert np.abs(back(dist.likelihood_ratio_sym(x, dict(prob=o), dict(prob=n_), axis=axis)) - lr).max() <= 1e-14
        assert np.abs(back(dist.log_likelihood_sym(x, dict(prob=n_), axis=axis)) - logli).max() <= 1e-15
        assert np.abs(back(dist.entropy_sym(dict(prob=n_), axis=axis)) - ent).max() <= 1e-15


# -- host stepping --------------------------------------------------------------------------------------------------------------
def test_host_stepping_follows_the_definition():
    """reset / get_action / get_actions: the probabilities they report are those of dist_info_planes on the observations
    and the actions THEY sampled; prev_action is the one-hot of the previous sampled action, zeros at a path start."""
    S, A, H = 16, 4, 32
    pol = _policy(S, A, H)
    rng = np.random.RandomState(5)
    np.random.seed(11)
    T = 9
    obs = rng.randint(0, S, size=T)
    pol.reset()
    acts, probs, prevs = [], [], []
    for t in range(T):
        if t == 4:
            pol.reset()
        a, info = pol.get_action(int(obs[t]))
        assert isinstance(a, int) and 0 <= a < A and set(info) == {"prob", "prev_action"}
        assert info["prob"].shape == (A,) and info["prob"].dtype == np.float64 and abs(info["prob"].sum() - 1) <= 1e-12
        acts.append(a); probs.append(info["prob"]); prevs.append(info["prev_action"])
    onehot, probs, prevs = np.eye(A)[acts], np.array(probs), np.array(prevs)
    assert len(set(acts)) > 1
    assert np.all(prevs[0] == 0) and np.all(prevs[4] == 0)
    assert np.array_equal(prevs[1:4], onehot[0:3]) and np.array_equal(prevs[5:], onehot[4:-1])
    start = np.zeros((T, 1), dtype=bool)
    start[[0, 4]] = True
    d = _planes(pol, np.eye(S)[obs].T[:, :, None].copy(), onehot.T[:, :, None].copy(), start, _flat64(pol))
    assert np.abs(d[:, :, 0].t().cpu().numpy() - probs).max() <= 1e-12
    # weighted_sample: the action is the cumulative rule on ONE np.random uniform
    pol.reset()
    np.random.seed(3)
    a, info = pol.get_action(0)
    np.random.seed(3)
    assert a == min(int((np.cumsum(info["prob"]) < np.random.rand()).sum()), A - 1)
    # the vectorised form: reset(dones) puts back the rows that are done and no others
    h0 = pol.get_param_values()[:H]
    pol.reset(dones=[True, True, True])
    assert np.array_equal(pol._prev_hiddens, np.tile(h0, (3, 1)))
    o3 = [1, 5, 9]
    a1, i1 = pol.get_actions(o3)
    assert len(a1) == 3 and np.all(i1["prev_action"] == 0) and i1["prob"].shape == (3, A)
    hidden = pol._prev_hiddens.copy()
    pol.reset(dones=[False, True, False])
    assert np.array_equal(pol._prev_hiddens[1], h0) and np.array_equal(pol._prev_hiddens[[0, 2]], hidden[[0, 2]])
    a2, i2 = pol.get_actions(o3)
    assert np.array_equal(i2["prev_action"][[0, 2]], np.eye(A)[a1][[0, 2]]) and np.all(i2["prev_action"][1] == 0)
    assert np.array_equal(i2["prob"][1], i1["prob"][1]) and not np.array_equal(i2["prob"][0], i1["prob"][0])
    # without the previous action in the state: no such agent_info
    bare = _policy(S, A, H, state_include_action=False)
    assert set(bare.get_action(3)[1]) == {"prob"}


# -- pickle, aliases, refusals --------------------------------------------------------------------------------------------------
def test_pickle_round_trip_keeps_the_parameters():
    pol = _policy(16, 4, 20, state_include_action=False)
    clone = pickle.loads(pickle.dumps(pol))
    assert np.array_equal(clone.get_param_values(), pol.get_param_values())
    assert clone.hidden_dim == 20 and clone.state_info_keys == [] and clone.input_dim == 16
    assert [p.name for p in clone.get_params(trainable=True)] == ORDER[1:]
    v0 = pol.param_version()
    pol.set_param_values(pol.get_param_values() * 0.5)
    assert pol.param_version() != v0
    pol.note_raw_write()
    assert pol.param_version()[1] == 1


def test_alias_imports_resolve():
    from rllab.distributions.recurrent_categorical import RecurrentCategorical
    from rllab.policies.categorical_gru_policy import CategoricalGRUPolicy
    import rllab_amd.distributions.recurrent_categorical as dmod
    import rllab_amd.policies.categorical_gru_policy as pmod
    assert CategoricalGRUPolicy is pmod.CategoricalGRUPolicy and RecurrentCategorical is dmod.RecurrentCategorical
    assert isinstance(_policy().distribution, RecurrentCategorical)


def test_feature_network_is_refused():
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    with pytest.raises(NotImplementedError) as e:
        CategoricalGRUPolicy(_spec(16, 4), feature_network=object())
    assert "feature_network" in str(e.value)


def test_recurrent_categorical_policy_takes_its_own_branch_of_the_algorithms():
    """``npo_inputs`` hands a recurrent categorical batch over as dense [., T, N] planes with the path starts."""
    from rllab_amd.algos.npo import is_categorical, npo_inputs

    class Traj(object):
        pass
    pol = _policy()
    assert is_categorical(pol) and pol.recurrent
    tr = Traj()
    T, N, S, A = 3, 2, 16, 4
    tr.B, tr.categorical, tr.count = T * N, True, 5.0
    tr.obs, tr.actions, tr.means = torch.zeros(S, T, N), torch.zeros(A, T, N), torch.full((A, T, N), 0.25)
    tr.advantages = torch.ones(T, N)
    tr.valid = torch.tensor([[1, 1], [1, 1], [1, 0]], dtype=torch.bool)
    tr.tin = torch.tensor([[0, 0], [1, 0], [2, 1]], dtype=torch.int32)
    tr.obs_dim, tr.act_dim = S, A
    obs, act, adv, old, start, w, inv = npo_inputs(pol, dict(_traj=tr))
    assert obs is tr.obs and act is tr.actions and adv is tr.advantages and old is tr.means
    assert start.tolist() == [[True, True], [False, True], [False, False]]
    assert w.dtype == torch.float32 and w.tolist() == [[1, 1], [1, 1], [1, 0]] and float(inv) == 0.2


# -- the ABI ------------------------------------------------------------------------------------------------------------------
def test_rollout_struct_mirror_matches_the_compiled_header(tmp_path):
    """include/rllab_amd.h compiled as plain C (gcc): sizeof and every offsetof of rl_gridworld_gru_args equal the ctypes
    mirror's, and the entry point is bound."""
    from rllab_amd import _lib
    assert "rl_rollout_gridworld_gru" in _lib.SYMBOLS
    assert list(_lib.lib.rl_rollout_gridworld_gru.argtypes) == [ctypes.POINTER(_lib.GridWorldGruArgs), ctypes.c_void_p]
    cls, cname = _lib.GridWorldGruArgs, "rl_gridworld_gru_args"
    lines = ['#include "rllab_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f, _ in cls._fields_:
        lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, f
    # the env fields come in rl_gridworld_args' order
    env_fields = [f for f, _ in _lib.GridWorldArgs._fields_ if f not in ("prob", "reserved")]
    mine = [f for f, _ in cls._fields_]
    assert [f for f in mine if f in env_fields] == env_fields
    # argument errors come back as status codes before anything touches a device
    assert _lib.lib.rl_rollout_gridworld_gru(None, None) == -1 and b"null" in _lib.lib.rl_last_error()
    assert _lib.lib.rl_rollout_gridworld_gru(ctypes.byref(cls(n_envs=1, horizon=1, n_act=4, n_row=4, n_col=4, hidden=48)),
                                             None) == -1        # null pointers are found before the hidden width is read
