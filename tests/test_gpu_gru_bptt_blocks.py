"""The recurrent update kernels of both GRU families (csrc/gru_bptt.h, gru_bptt_kernels.hip,
categorical_gru_bptt_kernels.hip) measured PER PARAMETER BLOCK, and at the edges of their plan.

tests/test_gpu_gru_bptt.py and tests/test_gpu_categorical_gru_bptt.py compare every vector by one norm over all trainable
entries.  A GRU gradient, and a Fisher product along a dense direction, is dominated by b_out, W_out and the log-std row;
W_hr, the previous-action rows of W_x* and the sparse rows of a one-hot input carry a small share of that norm, so an error
confined to one of them stays under the whole-vector allowance.  Here the same rule -- the kernel's relative error against
float64 autograd is at most ALLOW = 8 x the float32 autograd's, the yardstick floored at FLOOR = 2^-20 -- is applied to
every block on the block's own norm.  A block is one trainable parameter as ``get_params(trainable=True)`` lists it, each
W_x* cut into its observation rows and its previous-action rows.  The helpers, closures and cached references are the two
sibling modules'.

A  the gradient and the three Fisher products of every entry of both CASES lists, per block.
B  Fisher products along directions supported in ONE block, compared per output block: the coupling of two light blocks.
C  past the cap of the weight sums' sample chunks (B = T N > 32768).
D  lane counts 64, 65, 128; T = 2; hidden widths 1, 33, 63 (Gaussian) and 1, 31 (categorical).
E  saturated gates.
F  the same bits twice at the plan of C.

A block where the KERNEL's value is zero by construction is named in ``zero``: the previous-action rows at T = 1 (no step
has a previous action: the reference is exactly zero too) and, in B, the coupling of the log-std row with everything else
(at new == old it vanishes; the kernels do not compute it, and the float64 reference holds there only what the float32
old means differ by from the float64 new ones).  Such a block must hold exact zeros and the reference's block at most
ALLOW x FLOOR of the whole reference's norm; it is not compared by the rule (there is no norm to divide by).
"""
import numpy as np
import pytest
import torch

import test_gpu_categorical_gru_bptt as C
import test_gpu_gru_bptt as G

pytestmark = pytest.mark.gpu

FLOOR, ALLOW = G.FLOOR, G.ALLOW
assert (C.FLOOR, C.ALLOW) == (FLOOR, ALLOW) == (2.0 ** -20, 8.0)
SAT = 2.0 ** -20
_VALUE = [("value", 0, 1)]


def _fam(case):
    return G if isinstance(case[0], int) else C


def _blocks(pol):
    """[(name, begin, end)] in the flat order: the trainable parameters, W_x* cut behind its observation rows."""
    out = []
    for p in pol.get_params(trainable=True):
        if p.name.startswith("W_x") and pol.state_include_action:
            cut = p.offset + pol.obs_dim * pol.hidden_dim
            out += [(p.name + ".obs", p.offset, cut), (p.name + ".act", cut, p.offset + p.size)]
        else:
            out.append((p.name, p.offset, p.offset + p.size))
    assert sum(e - b for _, b, e in out) == sum(p.size for p in pol.get_params(trainable=True))
    return out


def _within_blocks(name, got, ref64, ref32, blocks, zero=()):
    """The rule of the two sibling modules on every block's own norm: e_k(block) <= ALLOW max(e_32(block), FLOOR).
    ``ref32``: the float32 autograd's vector, or several evaluations of it (the yardstick is then the largest error).
    One line per block; every block is looked at before the first failure is raised."""
    refs32 = ref32 if isinstance(ref32, (list, tuple)) else (ref32,)
    whole = float(ref64.norm())
    bad = []
    for bname, b, e in blocks:
        x, r = got[b:e], ref64[b:e]
        n64 = float(r.norm())
        if bname in zero:
            ok = bool(torch.all(x == 0)) and n64 <= ALLOW * FLOOR * whole
            print("%s [%s]: zero by construction, kernel max %.3e, float64 block norm %.3e of %.3e" % (
                name, bname, float(x.abs().max()), n64, whole))
        else:
            assert n64 > 0 and np.isfinite(n64), (name, bname, n64)        # nothing is compared vacuously
            e_k = float((x - r).norm()) / n64
            e_32 = max(float((y[b:e] - r).norm()) / n64 for y in refs32)
            ok = e_k <= ALLOW * max(e_32, FLOOR)
            print("%s [%s]: kernel %.3e, float32 autograd %.3e, ratio to the floored yardstick %.2f" % (
                name, bname, e_k, e_32, e_k / max(e_32, FLOOR)))
        if not ok:
            bad.append(bname)
    assert not bad, (name, bad)


_OWN = {}


def _ref(case, scale=0.1, **planes_kw):
    """``_case`` of the family's module (its cache) for planes as ``_planes`` makes them; for a policy scale or planes of
    this module's own the same record, computed once here.  Never written to."""
    mod = _fam(case)
    if scale == 0.1 and not planes_kw:
        r = mod._case(case)
        r.setdefault("planes_kw", {})
        return r
    key = (case, scale, tuple(sorted((k, getattr(v, "__name__", v)) for k, v in planes_kw.items())))
    if key in _OWN:
        return _OWN[key]
    kind, hidden, N, T, inc = case
    pol = mod._policy(kind, hidden, scale=scale, state_include_action=inc)
    pol = pol[1] if isinstance(pol, tuple) else pol
    ops = pol.fused_ops()
    assert ops is not None, pol.why_no_kernel_layout()
    inputs = mod._planes(pol, N, T, **planes_kw)
    assert ops.accepts(inputs)
    surr, kl = mod._closures(pol)
    r = dict(pol=pol, ops=ops, inputs=inputs, idx=pol._flat_index(trainable=True), planes_kw=planes_kw)
    r["l64"], r["g64"] = mod._grad(pol, surr, inputs, torch.float64)
    r["l32"], r["g32"] = mod._grad(pol, surr, inputs, torch.float32)
    with torch.no_grad():
        r["k64"] = kl(pol.flat_params.detach().double(), *mod._cast(inputs, torch.float64)).double()
        r["k32"] = kl(pol.flat_params.detach(), *inputs).double()
    _OWN[key] = r
    return r


def _pad_mask(ops, dev):
    pad = torch.ones(ops.n_kernel, dtype=torch.bool, device=dev)
    if ops.index is None:
        pad[:] = False
    else:
        pad[ops.index] = False
    return pad


def _zero_rows(case, blocks):
    """The previous-action rows at T = 1: every step starts a path."""
    return {n for n, _, _ in blocks if case[3] == 1 and n.endswith(".act")}


def _sums_and_gradient(case, r, sums=True):
    """Loss, KL and the gradient of a case under the rule, the gradient per block.  -> the gradient in the flat order."""
    pol, ops, inputs = r["pol"], r["ops"], r["inputs"]
    blocks = _blocks(pol)
    ops.release()
    gk = ops.loss_grad_kernel(inputs, with_loss=True)
    loss, kl = ops.loss_and_kl(inputs)
    assert np.isfinite(loss) and np.isfinite(kl) and bool(torch.isfinite(gk).all())
    if sums:
        t = lambda x: torch.as_tensor([x], dtype=torch.float64)
        _within_blocks("loss %r" % (case,), t(loss), r["l64"].cpu().reshape(1), r["l32"].cpu().reshape(1), _VALUE)
        _within_blocks("KL %r" % (case,), t(kl), r["k64"].cpu().reshape(1), r["k32"].cpu().reshape(1), _VALUE)
    assert bool(torch.all(gk[:pol.kernel_hidden] == 0)) and bool(torch.all(gk[_pad_mask(ops, gk.device)] == 0))
    g = ops.gather(gk).double()
    _within_blocks("gradient %r" % (case,), g, r["g64"], r["g32"], blocks, _zero_rows(case, blocks))
    return g


def _direction(r, x):
    """x at the trainable entries, zero at h0."""
    v = torch.zeros_like(r["g64"])
    v[r["idx"]] = x.to(v.dtype)[r["idx"]]
    return v


def _fisher(case, r, dirs, zero=None):
    """F x for every (name, x) of ``dirs`` against the float64 Perlmutter product, per output block; the float32 products
    of the yardstick come from one graph, like the float64 ones.  ``zero``: name -> the blocks that are zero by
    construction (next to the previous-action rows at T = 1).  -> {name: F x in the kernel layout}."""
    mod = _fam(case)
    pol, ops = r["pol"], r["ops"]
    blocks = _blocks(pol)
    inputs = mod._planes(pol, case[2], case[3], at_old=True, **r["planes_kw"])
    _, kl = mod._closures(pol)
    vs = [x for _, x in dirs]
    H64 = mod._hvp(pol, kl, inputs, torch.float64, vs)
    H32 = mod._hvp(pol, kl, inputs, torch.float32, vs)
    ops.release()
    pad = _pad_mask(ops, vs[0].device)
    out = {}
    for (name, x), h64, h32 in zip(dirs, H64, H32):
        fk = ops.fvp_kernel(inputs, ops.scatter(x))
        assert bool(torch.isfinite(fk).all())
        assert bool(torch.all(fk[:pol.kernel_hidden] == 0)) and bool(torch.all(fk[pad] == 0))     # h0; the padded places
        got = ops.gather(fk).double()
        z = _zero_rows(case, blocks) | set((zero or {}).get(name, ()))
        _within_blocks("F %s %r" % (name, case), got, h64, h32, blocks, z)
        assert float(x.dot(got)) > 0, name
        out[name] = fk
    ops.release()
    return out


# -- A. every case of the two modules, per block ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES + C.CASES)
def test_gradient_per_block(case):
    _sums_and_gradient(case, _ref(case), sums=False)


@pytest.mark.parametrize("case", G.CASES + C.CASES)
def test_fisher_products_per_block(case):
    """The three directions of the sibling modules' Fisher test: two dense random ones and the gradient."""
    r = _ref(case)
    n, dev = r["g64"].numel(), r["g64"].device
    rng = np.random.RandomState(11)
    u = _direction(r, torch.as_tensor(rng.randn(n), device=dev))
    v = _direction(r, torch.as_tensor(rng.randn(n), device=dev))
    _fisher(case, r, [("u", u), ("v", v), ("g", _direction(r, r["g64"]))])


# -- B. directions supported in one block ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 20, 70, 25, True), ("chain", 32, 70, 25, True)])
def test_fisher_products_of_block_supported_directions(case):
    """For every block b a direction that is random inside b (seeded by b's index) and zero elsewhere; F v_b per OUTPUT
    block: row b of the block matrix of F, so a wrong coupling of two light blocks is a whole block's error.  (13, 2) at
    20 units: padding, two actions, previous-action rows; chain at 32: a partial second row block of [x; 1].
    The log-std row couples with nothing else at new == old: those blocks are the ``zero`` ones of the module docstring."""
    r = _ref(case)
    blocks = _blocks(r["pol"])
    names = [n for n, _, _ in blocks]
    dirs, zero = [], {}
    for k, (name, b, e) in enumerate(blocks):
        v = torch.zeros_like(r["g64"])
        v[b:e] = torch.as_tensor(np.random.RandomState(100 + k).randn(e - b), device=v.device)
        dirs.append((name, v))
        if "log_std" in name:
            zero[name] = [m for m in names if m != name]
        else:
            zero[name] = [m for m in names if "log_std" in m]
    _fisher(case, r, dirs, zero)


# -- C., F. past the cap of the sample chunks ----------------------------------------------------------------------------------
N_C, T_C = 1573, 21
CASES_C = [(0, 32, N_C, T_C, True), ("4x4", 32, N_C, T_C, True)]


def _edit_c(start, w):
    """The special columns ``_planes`` makes only for T >= 25, for T = 21."""
    T = start.shape[0]
    start[T - 1, 1] = True                        # a start in the last row
    start[5:7, 0] = True                          # two consecutive starts: a path of length 1
    start[:, 2] = False                           # a column with no start after row 0
    start[14, 3] = True                           # weights 0 behind row 15: the rows behind a path that ended
    w[16:, 3] = 0.0


def _plan(N, T):
    """bptt_workspace's sample chunks (csrc/gru_bptt.h): (B, chunks, L, lane workgroups)."""
    B = N * T
    chunks = min(-(-B // 128), 256)
    return B, chunks, 2 * (-(-B // (2 * chunks))), -(-N // 64)


def _replay(pol, obs, act, start, flat):
    """GRUPolicyBase._scan_planes restated step by step with the gates of gru_planes spelled out, so that x, h_prev, r, u
    and c of every step can be looked at.  -> (steps, heads [., T, N]); the callers compare the heads with the policy's
    own scan."""
    v = pol._views(flat)
    dt = flat.dtype
    obs, act = obs.to(dt), act.to(dt)
    T, N = obs.shape[1], obs.shape[2]
    h0 = v["h0"][:, None]
    h = h0.expand(h0.shape[0], N)
    zeros = torch.zeros((pol.action_dim, N), dtype=dt, device=obs.device)
    steps, heads = [], []
    for t in range(T):
        if t > 0:
            st = start[t][None, :]
            h = torch.where(st, h0, h)
        x = obs[:, t]
        if pol.state_include_action:
            x = torch.cat([x, zeros if t == 0 else torch.where(st, zeros, act[:, t - 1])], dim=0)
        rg = torch.sigmoid(v["W_xr"].t() @ x + v["W_hr"].t() @ h + v["b_r"][:, None])
        ug = torch.sigmoid(v["W_xu"].t() @ x + v["W_hu"].t() @ h + v["b_u"][:, None])
        cg = torch.tanh(v["W_xc"].t() @ x + rg * (v["W_hc"].t() @ h) + v["b_c"][:, None])
        steps.append(dict(x=x, h_prev=h, r=rg, u=ug, c=cg))
        h, head = pol.step_planes(x, h, v)
        heads.append(head)
    return steps, torch.stack(heads, dim=1)


def _head_of(mod, pol, inputs, flat):
    with torch.no_grad():
        d = pol.dist_info_planes(inputs[0], inputs[1], inputs[-3], flat)
    return d["mean"] if mod is G else d["prob"]


def _last_row_sum(mod, pol, inputs, lo):
    """float64: what the samples s >= ``lo`` -- all in the last row -- add to the weight sums: the gradient of their own
    loss terms in a second copy of the parameters that only their step reads (h_prev is a constant there), which is
    sum_s [x; 1; h_prev]_s (x) [dr; du; dc]_s and sum_s h'_s (x) dmean_s over those samples."""
    obs, act, adv, start, w, inv = inputs[0], inputs[1], inputs[2], inputs[-3], inputs[-2], inputs[-1]
    T, N = start.shape
    c0 = lo - (T - 1) * N
    assert 0 <= c0 < N
    flat = pol.flat_params.detach().double()
    with torch.no_grad():
        steps, heads = _replay(pol, obs[:, :, c0:], act[:, :, c0:], start[:, c0:], flat)
    assert torch.allclose(heads, _head_of(mod, pol, inputs, flat)[:, :, c0:], rtol=1e-10, atol=1e-13)
    leaf = flat.clone().requires_grad_(True)
    v = pol._views(leaf)
    _, head = pol.step_planes(steps[T - 1]["x"], steps[T - 1]["h_prev"], v)
    head, a = head[:, None, :], act[:, T - 1:, c0:].double()
    if mod is G:
        old = dict(mean=inputs[3][:, T - 1:, c0:].double(), log_std=inputs[4].double())
        new = dict(mean=head, log_std=v["output_log_std.param"][:, None, None])
    else:
        old, new = dict(prob=inputs[3][:, T - 1:, c0:].double()), dict(prob=head)
    lr = pol.distribution.likelihood_ratio_sym(a, old, new, axis=0)
    loss = -(lr * adv[T - 1:, c0:].double() * w[T - 1:, c0:].double()).sum() * inv.to(lr.dtype)
    return torch.autograd.grad(loss, leaf)[0]


def _case_c(case):
    return _ref(case, edit=_edit_c)


@pytest.mark.parametrize("case", CASES_C)
def test_past_the_chunk_cap(case):
    """N = 1573, T = 21: B = 33 033 samples (odd) > 32 768, so the weight sums run 256 chunks -- the cap -- of L = 130
    samples.  Chunk 254 holds the last 13 samples (33 020 .. 33 032), chunk 255 starts at 33 150 > B and must add exact
    zeros; gru_finish_kernel folds 256 float32 partial rows per parameter; the sweeps run 25 lane workgroups, the last
    with 37 live lanes.  A change of the plan changes these numbers: they are recomputed below from bptt_workspace's
    formulas.
    The weight blocks are also rebuilt from the float64 sum over the first 33 020 samples alone: that vector misses the
    full reference by more than the kernel does, and by more than the rule allows, so a dropped tail chunk cannot pass."""
    mod = _fam(case)
    B, chunks, L, lanes = _plan(N_C, T_C)
    assert (B, chunks, L, lanes, N_C - 64 * (lanes - 1)) == (33033, 256, 130, 25, 37)
    assert B % 2 == 1 and B > 32768 and L > 128
    last = (B - 1) // L                                    # the last chunk that holds a sample
    assert (last, last * L, (chunks - 1) * L) == (254, 33020, 33150) and (chunks - 1) * L > B
    r = _case_c(case)
    pol, inputs = r["pol"], r["inputs"]
    start, w = inputs[-3], inputs[-2]
    assert bool(start[T_C - 1, 1]) and bool(start[5, 0]) and bool(start[6, 0]) and float(w[16:, 3].abs().max()) == 0
    g = _sums_and_gradient(case, r)
    _fisher(case, r, [("g", _direction(r, r["g64"]))])
    # the tail chunk: samples 33 020 .. 33 032 sit in the last row, with weight, and not all of them start a path
    lo = last * L
    c0 = lo - (T_C - 1) * N_C
    assert float(w[T_C - 1, c0:].min()) > 0 and not bool(start[T_C - 1, c0:].all())
    tail = _last_row_sum(mod, pol, inputs, lo)
    for name, b, e in _blocks(pol):
        if not name.startswith(("W_x", "W_h", "output.W")):
            continue
        n64 = float(r["g64"][b:e].norm())
        miss = float(tail[b:e].norm()) / n64               # ||(g64 - tail) - g64|| / ||g64||
        e_k = float((g[b:e] - r["g64"][b:e]).norm()) / n64
        e_32 = float((r["g32"][b:e] - r["g64"][b:e]).norm()) / n64
        print("first %d samples only %r [%s]: misses by %.3e; kernel %.3e, bound %.3e" % (
            lo, case, name, miss, e_k, ALLOW * max(e_32, FLOOR)))
        assert miss > e_k and miss > ALLOW * max(e_32, FLOOR), name


@pytest.mark.parametrize("case", CASES_C)
def test_twice_the_same_bits_past_the_chunk_cap(case):
    """test_every_pass_twice_gives_the_same_bits at 256 chunks and 25 lane workgroups."""
    r = _case_c(case)
    ops, inputs = r["ops"], r["inputs"]
    v = torch.as_tensor(np.random.RandomState(2).randn(ops.n_kernel).astype(np.float32), device=inputs[0].device)
    v = ops.scatter(ops.gather(v))
    v[:r["pol"].kernel_hidden] = 0.0
    ops.release()
    g1 = ops.loss_grad_kernel(inputs).clone()
    s1 = ops._last_out2.clone()
    f1 = ops.fvp_kernel(inputs, v).clone()
    f2 = ops.fvp_kernel(inputs, v).clone()
    g2 = ops.loss_grad_kernel(inputs).clone()            # ... behind two products on the same workspace
    assert torch.equal(f1, f2) and torch.equal(g1, g2) and torch.equal(s1, ops._last_out2)
    assert torch.equal(ops.fvp_kernel(inputs, v), f1)
    assert float(g1.abs().max()) > 0 and float(f1.abs().max()) > 0 and bool(torch.isfinite(f1).all())
    ops.release()


# -- D. lanes, horizon, widths ---------------------------------------------------------------------------------------------------
def _edges(case):
    r = _ref(case)
    _sums_and_gradient(case, r)
    _fisher(case, r, [("g", _direction(r, r["g64"]))])
    return r


@pytest.mark.parametrize("case", [(0, 32, 64, 25, True), (0, 32, 65, 25, True), (0, 32, 128, 25, True),
                                  ("4x4", 32, 64, 25, True), ("4x4", 32, 65, 25, True), ("4x4", 32, 128, 25, True)])
def test_whole_wavefronts_and_one_lane_more(case):
    _edges(case)


@pytest.mark.parametrize("case", [(0, 32, 70, 2, True), ("4x4", 32, 70, 2, True)])
def test_two_rows(case):
    """T = 2: the shortest horizon at which the backward sweep's look-ahead start[s + n] and the reads of row s - n both
    act, with row 1 starting a path in some columns and continuing one in others."""
    start = _ref(case)["inputs"][-3]
    assert 0 < int(start[1].sum()) < case[2]
    _edges(case)


@pytest.mark.parametrize("case", [(0, 1, 70, 25, True), (0, 33, 70, 25, True), (0, 63, 70, 25, True),
                                  ("4x4", 1, 70, 25, True), ("4x4", 31, 70, 25, True)])
def test_padded_widths(case):
    """One real unit; 33 and 63 units in the 64-unit instantiation (31 and 1 padded units); 31 of 32.  The categorical
    kernels run 1 .. 32 units: at 33 and above the tangent sweep of the 4x4 map needs 182 304 bytes of LDS and
    rl_gru_categorical_workspace_bytes refuses (tests/test_gpu_categorical_gru_bptt.py checks that refusal), so the
    categorical widths stop at 31."""
    from rllab_amd import _lib
    kind, hidden, N, T, inc = case
    Hk = 32 if hidden <= 32 else 64
    if _fam(case) is G:
        q = _lib.env_query(kind)
        assert _lib.lib.rl_gru_workspace_bytes(N, T, q["obs_dim"], q["act_dim"], Hk, 1) > 0
    else:
        assert _lib.lib.rl_gru_categorical_workspace_bytes(N, T, 16, Hk, 1) > 0
        assert _lib.lib.rl_gru_categorical_workspace_bytes(N, T, 16, 64, 1) == 0
    r = _edges(case)                 # (exact zeros at every padded place of gradient and product: checked in there)
    pol, ops = r["pol"], r["ops"]
    assert pol.kernel_hidden == Hk and ops.n_kernel > ops.n_flat
    assert int(_pad_mask(ops, "cpu").sum()) == ops.n_kernel - ops.n_flat


# -- E. saturated gates ----------------------------------------------------------------------------------------------------------
# Chosen on the CPU from the float64 gates: obs x 8 saturates 0.041 / 0.041 / 0.263 of r / u / c (mean 0.115).  Parameters
# moved by 1.0 randn saturate 0.009 / 0.002 / 0.069 on the chain map (mean 0.026 < 0.1), by 1.25 randn 0.085; 1.5 gives
# 0.192 / 0.106 / 0.222 (mean 0.173), the smallest of the steps tried that clears a tenth.
OBS_SCALE_E, PARAM_SCALE_E = 8.0, 1.5


@pytest.mark.parametrize("case,kw", [((2, 32, 70, 25, True), dict(obs_scale=OBS_SCALE_E)),
                                     (("chain", 32, 70, 25, True), dict(scale=PARAM_SCALE_E))])
def test_saturated_gates(case, kw):
    """Observation planes x 8 (Gaussian), parameters moved by 1.5 randn instead of 0.1 (categorical): many r, u are 0 or 1
    and many c are +-1 to float32, where fsigmoid / ftanh evaluate exp2 at its overflow and underflow ends.  Everything
    stays finite and inside the per-block rule: the float32 autograd of the yardstick saturates the same way.  At least a
    tenth of the gate values recomputed in float64 lie within 2^-20 of 0, 1 or +-1 (a condition on the inputs)."""
    mod = _fam(case)
    r = _ref(case, **kw)
    pol, inputs = r["pol"], r["inputs"]
    flat = pol.flat_params.detach().double()
    with torch.no_grad():
        steps, heads = _replay(pol, inputs[0], inputs[1], inputs[-3], flat)
    assert torch.allclose(heads, _head_of(mod, pol, inputs, flat), rtol=1e-10, atol=1e-13)
    H = pol.hidden_dim
    sat = torch.stack([torch.stack([(s["r"][:H] < SAT) | (s["r"][:H] > 1 - SAT), (s["u"][:H] < SAT) | (s["u"][:H] > 1 - SAT),
                                    s["c"][:H].abs() > 1 - SAT]) for s in steps]).double().mean(dim=(0, 2, 3))
    print("saturated share of r, u, c %r: %s" % (case, [round(float(x), 3) for x in sat]))
    assert float(sat.mean()) >= 0.1
    _sums_and_gradient(case, r)
    _fisher(case, r, [("g", _direction(r, r["g64"]))])
