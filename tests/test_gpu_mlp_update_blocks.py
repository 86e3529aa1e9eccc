"""The update kernels of the feed-forward policies (csrc/policy_kernels.hip, policy_split_kernels.hip,
policy_split16_kernels.hip, policy_splith_kernels.hip, policy_csplit_kernels.hip, policy_wide_kernels.hip,
gaussian_head_kernels.hip, categorical_kernels.hip) measured PER PARAMETER BLOCK and PER INPUT ROW of the first layer.

tests/test_gpu_update_parity.py, test_gpu_wide_nets.py, test_gpu_fvp_split.py, test_gpu_csplit.py, test_gpu_adaptive_std.py,
test_gpu_policy_options.py and test_gpu_categorical.py compare every vector by one number over all entries (2e-5 of the
largest entry for a gradient, 5e-5 for a Fisher product).  Here the rule of tests/test_gpu_gru_bptt_blocks.py -- the
kernel's relative error against float64 autograd is at most ALLOW = 8 x the float32 autograd's, the yardstick floored at
FLOOR = 2^-20 -- is applied to every block on the block's own norm.  A block is one trainable parameter as
``get_params(trainable=True)`` lists it; ``hidden_0.W`` (of every network of the policy) is additionally cut into its
obs_dim input rows ``hidden_0.W.row<d>``.  The policies, batches, float64 closures and the variant switches are the
sibling modules'; the float32 yardstick is the same formulas (the policy's own ``dist_info_planes`` and distribution) run
in float32 on the same inputs, and is held to the sibling closures in float64 before it is used.

A  every family on the inputs it is tested on today: surrogate and log-likelihood gradients, the loss / KL / log-likelihood
   sums, F u, F v, F g; 32-sample tile edges of the narrow family.
B  observation dimensions of different size: column d of the observations times 2^-round(17 d / (obs_dim - 1)), in three
   orders, on every Fisher-product arithmetic built for the shape.
C  directions supported in one block (the block matrix of F), and directions whose bias block is 2^-12 of its weight
   matrix, the light part measured by linearity.
D  one-hot observations with state frequencies from 1/2 down to one sample in 4096, and states that never occur.
(What the module catches that the whole-vector modules pass, measured on mutated kernels: DESIGN.md section 3.4f.)

A block that is zero by construction is named in ``zero``: the coupling of the log-std row with everything else at
new == old (the kernels do not compute it), and the ``hidden_0.W`` rows of one-hot states that never occur.  Such a block
must hold exact zeros and the float64 block at most ALLOW x FLOOR of the whole reference's norm.
"""
import numpy as np
import pytest
import torch

from tests import test_gpu_adaptive_std as AS
from tests import test_gpu_categorical as CT
from tests import test_gpu_fvp_split as S
from tests import test_gpu_update_parity as U
from tests import test_gpu_wide_nets as W
from tests.test_gpu_gru_bptt import ALLOW, FLOOR
from tests.test_gpu_gru_bptt_blocks import _within_blocks

pytestmark = pytest.mark.gpu

assert (FLOOR, ALLOW) == (2.0 ** -20, 8.0)
_VALUE = [("value", 0, 1)]
B_FULL = 4096
SPAN = 17                # policy_splith_kernels.hip: "an observation down to 2^-17 of the batch maximum keeps every bit"


# -- families ------------------------------------------------------------------------------------------------------------------
# case = (family, obs_dim, act_dim, hidden[, std hidden]); "narrow": policy_pass_kernel<Net<...>> and the split products,
# "coop": policy_wide_kernels.hip / csplit_fvp_kernel, "adaptive": gaussian_head_kernels.hip, "cat": categorical_kernels.hip
def _policy(case):
    fam = case[0]
    if fam == "adaptive":
        return AS._policy(*case[1:])
    if fam == "cat":
        return CT._policy(*case[1:])
    hidden = case[3]
    if isinstance(hidden, int):
        return U._policy(case[1], case[2], hidden)
    return W._policy(case[1], case[2], tuple(hidden))


def _mod(case):
    return {"adaptive": AS, "cat": CT}.get(case[0], U)


def _inputs(case, pol, B, old_equals_new=False):
    return _mod(case)._inputs(pol, B, old_equals_new=old_equals_new)


def _ops(case, pol):
    ops = pol.fused_ops()
    assert ops is not None
    want = {"narrow": "FusedGaussianMLPOps", "coop": "FusedGaussianMLPOps", "adaptive": "FusedAdaptiveStdOps",
            "cat": "FusedCategoricalOps"}[case[0]]
    assert type(ops).__name__ == want, (case, type(ops).__name__)
    if case[0] in ("narrow", "coop"):
        assert ops.wide_kernels == (case[0] == "coop"), case         # the kernel family the case is meant to run
    return ops


def _old(case, inp, dt):
    if case[0] == "cat":
        return dict(prob=inp[3].to(dt))
    return dict(mean=inp[3].to(dt), log_std=inp[4].to(dt))


def _terms(case, pol):
    """surr, kl, vpg of the sibling modules' ``_closures`` in the dtype of ``flat`` (theirs cast everything to float64):
    the policy's own ``dist_info_planes`` and distribution on the inputs cast to that dtype."""
    dist = pol.distribution

    def parts(flat, inp):
        dt = flat.dtype
        return pol.dist_info_planes(inp[0].to(dt), flat), _old(case, inp, dt), inp[1].to(dt), inp[2].to(dt), \
            inp[-2].to(dt), inp[-1].to(dt)

    def surr(flat, *inp):
        new, old, act, adv, w, inv = parts(flat, inp)
        return -(dist.likelihood_ratio_sym(act, old, new, axis=0) * adv * w).sum() * inv

    def kl(flat, *inp):
        new, old, act, adv, w, inv = parts(flat, inp)
        return (dist.kl_sym(old, new, axis=0) * w).sum() * inv

    def vpg(flat, *inp):
        new, old, act, adv, w, inv = parts(flat, inp)
        return -(dist.log_likelihood_sym(act, new, axis=0) * adv * w).sum() * inv
    return surr, kl, vpg


def _grad(pol, fn, inp, dt):
    """-> (value, gradient) of ``fn`` at the policy's parameters in ``dt``, both as float64."""
    flat = pol.flat_params.detach().to(dt).requires_grad_(True)
    val = fn(flat, *inp)
    assert val.dtype == dt
    return val.detach().double().reshape(1), torch.autograd.grad(val, flat)[0].double()


def _at_old64(case, pol, inp):
    """The inputs with the old distribution recomputed in float64, so that old == new exactly (what
    tests/test_gpu_fvp_split.py::_f64_products does for the Gaussian family)."""
    with torch.no_grad():
        d = pol.dist_info_planes(inp[0].double(), pol.flat_params.detach().double())
    if case[0] == "cat":
        return inp[:3] + (d["prob"],) + inp[4:]
    ls = d["log_std"] if case[0] == "adaptive" else pol.effective_log_std().detach().double().reshape(-1, 1)
    return inp[:3] + (d["mean"], ls) + inp[5:]


def _products(case, pol, inp, vs, dt):
    """The Perlmutter products of the mean KL along ``vs`` from one graph, as float64.  float64: old == new exactly
    (the Gaussian family through ``_f64_products``); float32: the float32 inputs the kernels read."""
    if dt == torch.float64 and case[0] in ("narrow", "coop"):
        return [h.detach() for h in S._f64_products(pol, inp, vs)]
    _, kl, _ = _terms(case, pol)
    use = _at_old64(case, pol, inp) if dt == torch.float64 else inp
    flat = pol.flat_params.detach().to(dt).requires_grad_(True)
    g = torch.autograd.grad(kl(flat, *use), flat, create_graph=True)[0]
    return [torch.autograd.grad((g * v.to(dt)).sum(), flat, retain_graph=True)[0].double() for v in vs]


def _same_closures(case, pol, inp):
    """The dtype-generic terms ARE the sibling module's float64 closures."""
    theirs = _mod(case)._closures(pol)
    flat = pol.flat_params.detach().double()
    with torch.no_grad():
        for mine, ref in zip(_terms(case, pol), theirs):
            a, b = float(mine(flat, *inp)), float(ref(flat, *inp))
            assert abs(a - b) <= 1e-12 * max(abs(b), 1e-3), (case, a, b)


def _f32(x):
    """A float32-representable float64 vector: both sides are handed the same values (``fvp`` rounds anyway)."""
    return x.float().double()


def _blocks(pol, rows=True):
    """[(name, begin, end)]: the trainable parameters in the flat order, then the input rows of every hidden_0.W."""
    params = pol.get_params(trainable=True)
    assert sum(p.size for p in params) == pol.flat_params.numel()
    out = [(p.name, p.offset, p.offset + p.size) for p in params]
    firsts = [p for p in params if p.name.endswith("hidden_0.W")]
    assert firsts and firsts[0].offset == 0
    for p in firsts if rows else ():
        h, r = divmod(p.size, pol.obs_dim)
        assert r == 0
        out += [("%s.row%d" % (p.name, d), p.offset + d * h, p.offset + (d + 1) * h) for d in range(pol.obs_dim)]
    return out


def _rows(pol):
    return [b for b in _blocks(pol) if ".row" in b[0] and not b[0].startswith("std.")]


def _share(x, blocks):
    """Every block's share of the norm of x."""
    whole = float(x.norm())
    return [float(x[b:e].norm()) / whole for _, b, e in blocks]


def _e32(ref32, ref64, blocks):
    return [float((ref32[b:e] - ref64[b:e]).norm()) / float(ref64[b:e].norm()) for _, b, e in blocks]


# -- references: computed once per key, never written to -------------------------------------------------------------------------
_REFS = {}


def _ref(case, B=B_FULL, make=None, key=None, at_old=False):
    """The record of a case: policy, ops, the gradient inputs (old != new) with their float64 / float32 references, the
    product inputs (old == new).  ``make(case, pol, B, old_equals_new)``: inputs of the caller's own.  ``at_old``: one
    batch with old == new for both (a gradient pass that fills the cache of the products)."""
    k = (case, B, key)
    if k in _REFS:
        return _REFS[k]
    make = make or _inputs
    pol = _policy(case)
    inp_f = make(case, pol, B, True)
    r = dict(case=case, pol=pol, ops=_ops(case, pol), inp_g=inp_f if at_old else make(case, pol, B, False), inp_f=inp_f)
    assert r["ops"].accepts(r["inp_g"]) and r["ops"].accepts(r["inp_f"])
    _same_closures(case, pol, r["inp_g"])
    surr, kl, vpg = _terms(case, pol)
    for dt, s in ((torch.float64, "64"), (torch.float32, "32")):
        r["l" + s], r["g" + s] = _grad(pol, surr, r["inp_g"], dt)
        r["v" + s], r["gv" + s] = _grad(pol, vpg, r["inp_g"], dt)
        with torch.no_grad():
            r["k" + s] = kl(pol.flat_params.detach().to(dt), *r["inp_g"]).double().reshape(1)
    _REFS[k] = r
    return r


def _product_refs(r, name, dirs, inp=None):
    """{direction name: (v, F64 v, F32 v)}, kept with the record under ``name``."""
    if name not in r:
        inp = r["inp_f"] if inp is None else inp
        vs = [v for _, v in dirs]
        h64 = _products(r["case"], r["pol"], inp, vs, torch.float64)
        h32 = _products(r["case"], r["pol"], inp, vs, torch.float32)
        r[name] = {n: (v, a, b) for (n, v), a, b in zip(dirs, h64, h32)}
    return r[name]


def _dense(r):
    """Two dense normal directions and the float64 gradient, float32-representable."""
    n, dev = r["g64"].numel(), r["g64"].device
    rng = np.random.RandomState(11)
    u = torch.as_tensor(rng.randn(n).astype(np.float32), device=dev).double()
    v = torch.as_tensor(rng.randn(n).astype(np.float32), device=dev).double()
    return [("u", u), ("v", v), ("g", _f32(r["g64"]))]


def _t(x):
    return torch.as_tensor([x], dtype=torch.float64)


def _check_gradients(r, tag=""):
    """The three sums and both gradients of the record's gradient inputs under the rule."""
    case, pol, ops, inp = r["case"], r["pol"], r["ops"], r["inp_g"]
    blocks = _blocks(pol)
    ops.release()
    loss, kl = ops.loss_and_kl(inp)
    ll = ops.loglik_loss(inp)
    g = ops.loss_grad(inp).double()
    gv = ops.loss_grad(inp, vpg=True).double()
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(gv).all())
    bad = []
    for name, got, a, b, bl in (("loss", _t(loss), r["l64"].cpu(), r["l32"].cpu(), _VALUE),
                                ("KL", _t(kl), r["k64"].cpu(), r["k32"].cpu(), _VALUE),
                                ("log-likelihood loss", _t(ll), r["v64"].cpu(), r["v32"].cpu(), _VALUE),
                                ("gradient", g, r["g64"], r["g32"], blocks),
                                ("log-likelihood gradient", gv, r["gv64"], r["gv32"], blocks)):
        try:
            _within_blocks("%s%s %r" % (tag, name, case), got, a, b, bl)
        except AssertionError as e:                   # every vector is looked at before the first failure is raised
            bad.append(str(e))
    assert not bad, bad


def _check_products(r, refs, label, zero=None, take=None, positive=True):
    """F v of the kernel for every direction of ``refs`` under the rule, per output block."""
    case, pol, ops = r["case"], r["pol"], r["ops"]
    inp = take or r["inp_f"]
    blocks = _blocks(pol)
    bad = []
    for name, (v, h64, h32) in refs.items():
        got = ops.fvp(inp, v).double()
        assert bool(torch.isfinite(got).all()), (label, name)
        try:
            _within_blocks("%s F %s %r" % (label, name, case), got, h64, h32, blocks, set((zero or {}).get(name, ())))
        except AssertionError as e:
            bad.append(str(e))
        if positive:
            assert float(v.dot(got)) > 0, (label, name)
    assert not bad, bad


def _select(monkeypatch, case, split=None, wps=None):
    """The Fisher-product arithmetic of the launches that follow, by the switches of tests/test_gpu_fvp_split.py: the
    library's choice (``_arith`` "f16x2": variant 4 where it is built), "5" (``_arith`` "bf16x3": variant 1), or
    RLLAB_FVP_SPLIT / RLLAB_FVP_SPLIT_WPS as given.  -> the variant ``_arith`` promises, or None."""
    monkeypatch.delenv("RLLAB_FVP_SPLIT_WPS", raising=False)
    if split is None:
        return S._arith(monkeypatch, "f16x2", case[1:4]) if isinstance(case[3], int) and case[0] == "narrow" else \
            monkeypatch.delenv("RLLAB_FVP_SPLIT", raising=False)
    if split == "5":
        return S._arith(monkeypatch, "bf16x3", case[1:4])
    monkeypatch.setenv("RLLAB_FVP_SPLIT", split)
    if wps is not None:
        monkeypatch.setenv("RLLAB_FVP_SPLIT_WPS", wps)
    return None


# -- A. every family on the inputs it is tested on today, per block ---------------------------------------------------------
NARROW = [("narrow", 4, 1, 32), ("narrow", 13, 2, 32), ("narrow", 20, 6, 64), ("narrow", 21, 6, 64),
          ("narrow", 13, 2, (24, 20)),           # zero-padded to (32, 32)
          ("narrow", 13, 2, (20,))]              # one hidden layer: the kernel copy is (32, 32) with W1 = I
COOP = [("coop", 13, 2, (100, 50, 25)), ("coop", 20, 6, (128, 128)), ("coop", 6, 1, (40, 100, 40)), ("coop", 13, 2, (100,))]
ADAPTIVE = ("adaptive", 13, 2, (100, 50, 25), (20, 20))     # of test_gpu_adaptive_std.SHAPES: a cooperative mean network
assert ADAPTIVE[1:] in AS.SHAPES                            # and a zero-padded std network
CAT = [("cat", 16, 4, (32, 32)), ("cat", 29, 4, (100, 50, 25))]
CASES_A = NARROW + COOP + [ADAPTIVE] + CAT


def _id(case):
    return "-".join(str(c).replace(" ", "") for c in case)


@pytest.mark.parametrize("case", CASES_A, ids=_id)
def test_gradients_and_sums_per_block(case):
    _check_gradients(_ref(case))


@pytest.mark.parametrize("case", CASES_A, ids=_id)
def test_fisher_products_per_block(case, monkeypatch):
    """F u, F v, F g without the activation cache (the f32 matrix instructions: what the sibling modules' Perlmutter tests
    run) and behind a gradient pass that left it (what TRPO runs: the library's choice of arithmetic, printed)."""
    promised = _select(monkeypatch, case)
    r = _ref(case)
    ops, inp = r["ops"], r["inp_f"]
    refs = _product_refs(r, "dense", _dense(r))
    ops.release()
    assert S._variant(ops, inp) == 0
    _check_products(r, refs, "no cache, variant 0:")
    ops.loss_grad(inp, keep_activations=True)
    variant = S._variant(ops, inp)
    if promised is not None:
        assert variant == promised == 4 and ops._acts_tag is not None, case   # whole tiles, cached: the two-way f16 split
    _check_products(r, refs, "cached, variant %d:" % variant)
    ops.release()


EDGE_B = [1, 32, 33, 63, 4096, 4100]


@pytest.mark.parametrize("B", EDGE_B)
@pytest.mark.parametrize("case", [("narrow", 13, 2, 32), ("narrow", 20, 6, 64)], ids=_id)
def test_tile_edges_per_block(case, B, monkeypatch):
    """One sample, one tile, one tile and a sample, two tiles less one, 128 tiles, 128 tiles and four samples: partial
    tiles run the f32 product, whole tiles with cached activations the split product.  Gradient (which fills the cache)
    and F g at old == new."""
    assert _select(monkeypatch, case) == 4
    r = _ref(case, B=B, key="edge", at_old=True)
    pol, ops, inp = r["pol"], r["ops"], r["inp_f"]
    ops.release()
    g = ops.loss_grad(inp, keep_activations=True).double()
    want = 4 if B % 32 == 0 else 0
    assert S._variant(ops, inp) == want, (case, B)
    _within_blocks("gradient B = %d %r" % (B, case), g, r["g64"], r["g32"], _blocks(pol))
    refs = _product_refs(r, "g", [("g", _f32(r["g64"]))])
    _check_products(r, refs, "B = %d, variant %d:" % (B, want))
    ops.release()


# -- B. observation dimensions of different size, per input row ---------------------------------------------------------------
ORDERS = ["falling", "rising", "interleaved"]
_FAMILIES = ("narrow", "coop", "adaptive", "cat")


def _column(obs_dim, order):
    """2^-round(SPAN d / (obs_dim - 1)), d = 0 .. obs_dim - 1; reversed; or large / small alternating (the largest first,
    the smallest second, ...), so that the bias slot's neighbour row<obs_dim - 1> and row<0> are each once the heaviest
    and once the lightest."""
    e = [int(round(SPAN * d / (obs_dim - 1.0))) for d in range(obs_dim)]
    assert e[0] == 0 and e[-1] == SPAN
    if order == "rising":
        e = e[::-1]
    elif order == "interleaved":
        lo, hi, out = 0, obs_dim - 1, []
        while lo <= hi:
            out.append(e[lo])
            if lo != hi:
                out.append(e[hi])
            lo, hi = lo + 1, hi - 1
        e = out
    assert len(e) == obs_dim and min(e) == 0 and max(e) == SPAN
    return 2.0 ** -np.asarray(e, dtype=np.float64)


def _scaled(order):
    def make(case, pol, B, _old_equals_new):
        """``_inputs``' normal planes times the column; the old distribution recomputed from the scaled observations
        (float32, old == new: the gradient pass fills the cache the products read)."""
        col = torch.as_tensor(_column(pol.obs_dim, order).astype(np.float32), device=pol.flat_params.device)[:, None]
        if case[0] != "adaptive":
            return S._scaled_inputs(pol, B, col)
        inp = list(AS._inputs(pol, B, old_equals_new=True))
        inp[0] = inp[0] * col
        with torch.no_grad():
            d = pol.dist_info_planes(inp[0].double(), pol.flat_params.double())
        inp[3], inp[4] = d["mean"].float(), d["log_std"].float()
        return tuple(inp)
    return make


def _ref_b(case, order):
    """The record of section B with its conditions on the inputs, asserted from the references alone."""
    r = _ref(case, make=_scaled(order), key=order, at_old=True)
    if "cond" in r:
        return r
    pol = r["pol"]
    rows = _rows(pol)
    assert len(rows) == pol.obs_dim
    dirs = [("u", _dense(r)[0][1]), ("g", _f32(r["g64"]))]
    refs = _product_refs(r, "dense", dirs)
    obs = r["inp_f"][0]
    col = obs.abs().max(dim=1).values
    assert float(col.min()) < 2.0 ** (2 - SPAN) * float(col.max())
    light = min(_share(r["g64"], rows))
    print("B %r %s: lightest W0 row %.2e of the gradient's norm; float32 autograd per row %.2e .. %.2e" % (
        case, order, light, min(_e32(r["g32"], r["g64"], rows)), max(_e32(r["g32"], r["g64"], rows))))
    assert light <= 1e-5
    e = _e32(r["g32"], r["g64"], rows)
    assert np.all(np.isfinite(e)) and max(e) <= 1e-5, e
    for name, (v, h64, h32) in refs.items():
        light = min(_share(h64, rows))
        e = _e32(h32, h64, rows)
        print("B %r %s: lightest W0 row %.2e of the norm of F %s; float32 autograd per row %.2e .. %.2e" % (
            case, order, light, name, min(e), max(e)))
        assert light <= 1e-6, (name, light)
        assert np.all(np.isfinite(e)) and max(e) <= 1e-5, (name, e)
    r["cond"] = True
    return r


# (RLLAB_FVP_SPLIT, RLLAB_FVP_SPLIT_WPS, the variant rl_policy_fvp_variant must report)
ARITH_32 = [("0", None, 0), ("5", None, 1), (None, None, 4), ("3", "4", 3), ("3", "3", 3)]
ARITH_64 = [("0", None, 0), ("5", None, 1), (None, None, 4), ("2", None, 2)]
# every arithmetic of the two shapes in the three orders; the cooperative, the identity-layer and the adaptive_std shapes on
# the library's choice in the order at which the conditions on the inputs hold for them as the references stand (CPU,
# float64 / float32 autograd: with the scales rising the lightest gradient row of (13, 2, (20,)) holds 1.2e-5 of the norm,
# interleaved the float32 autograd misses one row of the adaptive_std mean network by 1.7e-5)
CASES_B = [(("narrow", 13, 2, 32), a, o) for a in ARITH_32 for o in ORDERS] + \
          [(("narrow", 20, 6, 64), a, o) for a in ARITH_64 for o in ORDERS] + \
          [(c, (None, None, None), "falling") for c in (("coop", 13, 2, (100, 50, 25)), ("narrow", 13, 2, (20,)), ADAPTIVE)]


@pytest.mark.parametrize("case,arith,order", CASES_B,
                         ids=lambda x: x if isinstance(x, str) else _id(x) if x[0] in _FAMILIES else "split%s-wps%s-v%s" % x)
def test_observation_dimensions_of_different_size(case, arith, order, monkeypatch):
    """Span 2^-17 over the observation dimensions: the gradient with the cache (and max |obs| of the batch), F u and F g
    per block and per W0 row, on the arithmetic ``arith``; the lightest row carries 1e-6 .. 1e-8 of a vector's norm."""
    split, wps, want = arith
    _select(monkeypatch, case)
    r = _ref_b(case, order)
    pol, ops, inp = r["pol"], r["ops"], r["inp_f"]
    ops.release()
    g = ops.loss_grad(inp, keep_activations=True).double()
    if case[0] == "narrow":
        assert float(ops._absmax) == float(inp[0].abs().max())
    promised = _select(monkeypatch, case, split, wps)
    variant = S._variant(ops, inp)
    if want is not None:
        assert variant == want and promised in (None, want), (case, arith, variant)     # the launches below ARE that kernel
    bad = []
    try:
        _within_blocks("B %s gradient %r" % (order, case), g, r["g64"], r["g32"], _blocks(pol))
    except AssertionError as e:
        bad.append(str(e))
    try:
        _check_products(r, r["dense"], "B %s variant %d:" % (order, variant))
    except AssertionError as e:
        bad.append(str(e))
    ops.release()
    assert not bad, bad


# -- C. directions supported in one block, and in part of one ---------------------------------------------------------------
CASES_C = [(("narrow", 13, 2, 32), None, 4), (("narrow", 13, 2, 32), "5", 1), (("narrow", 20, 6, 64), None, 4)]


def _cached(r, split, want, monkeypatch):
    _select(monkeypatch, r["case"])
    ops, inp = r["ops"], r["inp_f"]
    ops.release()
    ops.loss_grad(inp, keep_activations=True)
    assert _select(monkeypatch, r["case"], split) == want
    assert S._variant(ops, inp) == want


@pytest.mark.parametrize("case,split,want", CASES_C, ids=lambda x: _id(x) if isinstance(x, tuple) else str(x))
def test_block_supported_directions(case, split, want, monkeypatch):
    """For every block b (every parameter and every W0 row) a direction that is normal inside b (seeded by b's index)
    and zero elsewhere; F v_b per OUTPUT block: row b of the block matrix of F.  A direction supported only in b0, or only
    in W2, leaves two of the three |v| maxima of ``block_maxima`` at zero and their exponents at the -30 floor of
    ``exp_of``.  The log-std row couples with nothing else at new == old: the ``zero`` blocks."""
    r = _ref(case)
    blocks = _blocks(r["pol"])
    names = [n for n, _, _ in blocks]
    dirs, zero = [], {}
    for k, (name, b, e) in enumerate(blocks):
        v = torch.zeros_like(r["g64"])
        v[b:e] = torch.as_tensor(np.random.RandomState(100 + k).randn(e - b).astype(np.float32), device=v.device).double()
        dirs.append((name, v))
        zero[name] = [m for m in names if ("log_std" in m) != ("log_std" in name)]
    refs = _product_refs(r, "blocks", dirs)
    _cached(r, split, want, monkeypatch)
    _check_products(r, refs, "C variant %d:" % want, zero=zero)
    r["ops"].release()


@pytest.mark.parametrize("case,split,want", CASES_C, ids=lambda x: _id(x) if isinstance(x, tuple) else str(x))
def test_light_bias_next_to_its_weight_matrix(case, split, want, monkeypatch):
    """b0 (resp. b1) normal x 2^-12 while W0 (resp. W1) is normal x 1, everything else zero: the two share one scale in
    ``make_scales``.  F is linear, so F v - F v_heavy (v_heavy: the bias block zeroed; both products by the kernel) is
    F v_light, compared with the float64 F v_light on ITS norm; the float32 yardstick of the difference is formed the
    same way from two float32 autograd products."""
    r = _ref(case)
    pol, ops, inp = r["pol"], r["ops"], r["inp_f"]
    by = {n: (b, e) for n, b, e in _blocks(pol, rows=False)}
    if "light" not in r:
        rec = {}
        for k, layer in enumerate(("hidden_0", "hidden_1")):
            rng = np.random.RandomState(200 + k)
            (wb, we), (bb, be) = by[layer + ".W"], by[layer + ".b"]
            heavy, light = torch.zeros_like(r["g64"]), torch.zeros_like(r["g64"])
            heavy[wb:we] = torch.as_tensor(rng.randn(we - wb).astype(np.float32), device=heavy.device).double()
            light[bb:be] = torch.as_tensor(rng.randn(be - bb).astype(np.float32), device=heavy.device).double() * 2.0 ** -12
            full = heavy + light
            assert torch.equal(_f32(full), full)
            (l64,) = _products(case, pol, inp, [light], torch.float64)
            f32, h32 = _products(case, pol, inp, [full, heavy], torch.float32)
            rec[layer] = (full, heavy, l64, f32 - h32)
        r["light"] = rec
    _cached(r, split, want, monkeypatch)
    zero = {n for n, _, _ in _blocks(pol) if "log_std" in n}
    bad = []
    for layer, (full, heavy, l64, d32) in r["light"].items():
        got = ops.fvp(inp, full).double() - ops.fvp(inp, heavy).double()
        try:
            _within_blocks("C variant %d: F v - F v_heavy, light %s.b %r" % (want, layer, case), got, l64, d32,
                           _blocks(pol), zero)
        except AssertionError as e:
            bad.append(str(e))
    ops.release()
    assert not bad, bad


# -- D. one-hot observations ------------------------------------------------------------------------------------------------------
CASE_D = ("cat", 16, 4, (32, 32))
N_SEEN = 12              # states 0 .. 11 occur with probability ~ 2^-s, states 12 .. 15 never
SEED_D = 2               # chosen on the CPU: state 11 occurs once with weight 1 in both batches below


def _one_hot(case, pol, B, old_equals_new):
    """``_inputs``' batch with one-hot observation planes (what FusedCategoricalOps.accepts documents) and the old
    probabilities built from THEM as ``_inputs`` builds its own: the current ones, or the current logits moved by
    0.05 N(0, 1)."""
    inp = list(CT._inputs(pol, B, old_equals_new=old_equals_new))
    rng = np.random.RandomState(1000 + SEED_D)
    p = 2.0 ** -np.arange(N_SEEN)
    state = rng.choice(N_SEEN, size=B, p=p / p.sum())
    dev = inp[0].device
    inp[0] = torch.as_tensor(np.eye(pol.obs_dim, dtype=np.float32)[state].T.copy(), device=dev)
    with torch.no_grad():
        logits = pol.logit_planes(inp[0].double(), pol.flat_params.double())
        if not old_equals_new:
            logits = logits + 0.05 * torch.as_tensor(rng.randn(pol.action_dim, B), device=dev)
        inp[3] = torch.softmax(logits, dim=0).float()
    return tuple(inp)


def test_one_hot_observations_per_state_row():
    """Gradient and F g per block and per W0 row; row s sums over the samples of state s alone: 2048 of them for state 0,
    about one for state 11, none for 12 .. 15 (exact zeros on both sides)."""
    r = _ref(CASE_D, make=_one_hot, key="one-hot")
    pol, ops = r["pol"], r["ops"]
    blocks = _blocks(pol)
    never = {"hidden_0.W.row%d" % s for s in range(N_SEEN, pol.obs_dim)}
    refs = _product_refs(r, "g", [("g", _f32(r["g64"]))])
    for inp in (r["inp_g"], r["inp_f"]):
        obs, w = inp[0], inp[-2]
        assert bool(torch.all((obs == 0) | (obs == 1))) and bool(torch.all(obs.sum(dim=0) == 1))
        count = (obs * w[None, :]).sum(dim=1)
        print("D: weighted samples per state %s" % [int(c) for c in count])
        assert float(count[N_SEEN - 1]) >= 1 and float(count[N_SEEN:].abs().max()) == 0
    for name, b, e in blocks:
        if name in never:
            assert bool(torch.all(r["g64"][b:e] == 0)) and bool(torch.all(refs["g"][1][b:e] == 0)), name
    ops.release()
    g = ops.loss_grad(r["inp_g"]).double()
    _within_blocks("D gradient %r" % (CASE_D,), g, r["g64"], r["g32"], blocks, never)
    _check_products(r, refs, "D:", zero={"g": never})
    ops.release()
