"""Restatements the DDPG tests measure against (shared by test_ddpg_host.py and test_gpu_ddpg_update.py; no test here).

``restated_update`` is one DDPG update (rllab/algos/ddpg.py:331-365 with the closures of init_opt, :267-329) as torch
expressions on the CPU, gradients by AUTOGRAD, in the dtype asked for -- independent of the kernel's hand-derived
backward pass and of the product's forward code (the networks are written out here from the flat parameter vectors:
W0 b0 W1 b1 W2 b2, W stored [in, out], Q's W1 = hidden rows then action rows).  ``draw_rows`` is the batch-index rule of
rl_ddpg_update in numpy on ``oracle.host_env.philox`` words.

The accuracy rule is the project's (tests/test_gpu_gru_bptt.py): per block, on the block's own norm, the error against
float64 is at most ALLOW x the float32 restatement's, the yardstick floored at FLOOR.
"""
import numpy as np
import torch

FLOOR = 2.0 ** -20
ALLOW = 8.0
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

# (D, A, hidden, hidden activation, B) of the issue
SHAPES = [(4, 1, (32, 32), "rectify", 32), (21, 6, (64, 64), "tanh", 32), (13, 2, (20, 7), "rectify", 33),
          (4, 1, (64, 32), "tanh", 1), (20, 6, (32, 64), "rectify", 128)]
POOL_ROWS = 512


def layer_shapes(D, A, hs, merge, out):
    h0, h1 = hs
    return [("W0", (D, h0)), ("b0", (h0,)), ("W1", (h0 + merge, h1)), ("b1", (h1,)), ("W2", (h1, out)), ("b2", (out,))]


def blocks(D, A, hs, merge, out, prefix=""):
    """[(name, begin, end)] of a net's flat vector."""
    res, off = [], 0
    for name, shape in layer_shapes(D, A, hs, merge, out):
        n = int(np.prod(shape))
        res.append((prefix + name, off, off + n))
        off += n
    return res


def split(flat, D, A, hs, merge, out):
    return [flat[b:e].reshape(shape) for (_, b, e), (_, shape) in zip(blocks(D, A, hs, merge, out),
                                                                     layer_shapes(D, A, hs, merge, out))]


def _act(name):
    return {"rectify": torch.relu, "tanh": torch.tanh, None: (lambda x: x)}[name]


def pi_forward(flat, s, cfg):
    W0, b0, W1, b1, W2, b2 = split(flat, cfg["D"], cfg["A"], cfg["hs"], 0, cfg["A"])
    f = _act(cfg["hact"])
    return _act(cfg["oact"])(f(f(s @ W0 + b0) @ W1 + b1) @ W2 + b2)


def q_forward(flat, s, a, cfg):
    W0, b0, W1, b1, W2, b2 = split(flat, cfg["D"], cfg["A"], cfg["hs"], cfg["A"], 1)
    f = _act(cfg["hact"])
    return (f(torch.cat([f(s @ W0 + b0), a], dim=1) @ W1 + b1) @ W2 + b2).reshape(-1)


def weight_mask(D, A, hs, merge, out):
    m = []
    for name, shape in layer_shapes(D, A, hs, merge, out):
        m.append(torch.full((int(np.prod(shape)),), 1.0 if name.startswith("W") else 0.0, dtype=torch.float64))
    return torch.cat(m)


def make_cfg(D, A, hs, hact, B, oact="tanh", **kw):
    cfg = dict(D=D, A=A, hs=tuple(hs), hact=hact, oact=oact, B=B, discount=0.99, tau=0.01, qf_lr=1e-3, pi_lr=1e-4,
               qf_wd=0.0, pi_wd=0.0, qf_method="sgd", pi_method="sgd")
    cfg.update(kw)
    return cfg


def make_state(cfg, seed=0, scale=0.2):
    """Parameters of both nets with every block -- biases too -- off zero, targets a little away from them, moments 0.
    float64 tensors that are float32 values (so that every dtype starts from the same numbers)."""
    rng = np.random.RandomState(seed)
    D, A, hs = cfg["D"], cfg["A"], cfg["hs"]
    n_pi = blocks(D, A, hs, 0, A)[-1][2]
    n_q = blocks(D, A, hs, A, 1)[-1][2]
    f = lambda n, s: torch.as_tensor((s * rng.randn(n)).astype(np.float32)).double()
    st = dict(pi=f(n_pi, scale), q=f(n_q, scale))
    st["tpi"] = (st["pi"] + f(n_pi, 0.05)).float().double()
    st["tq"] = (st["q"] + f(n_q, 0.05)).float().double()
    for k, n in (("m_pi", n_pi), ("v_pi", n_pi), ("m_q", n_q), ("v_q", n_q)):
        st[k] = torch.zeros(n, dtype=torch.float64)
    st["t_pi"] = st["t_q"] = 0
    return st


def make_pool(cfg, seed=1, rows=POOL_ROWS, term_frac=0.1):
    rng = np.random.RandomState(seed)
    f = lambda *s: torch.as_tensor(rng.randn(*s).astype(np.float32))
    return dict(obs=f(rows, cfg["D"]), act=torch.as_tensor(rng.uniform(-1, 1, (rows, cfg["A"])).astype(np.float32)),
                rew=f(rows), term=torch.as_tensor((rng.rand(rows) < term_frac).astype(np.float32)),
                next_obs=f(rows, cfg["D"]), skip=torch.zeros(rows))


def make_indices(cfg, K, seed=2, rows=POOL_ROWS):
    return torch.as_tensor(np.random.RandomState(seed).randint(0, rows, size=(K, cfg["B"])).astype(np.int32))


def _step(theta, grad, m, v, t, method, lr, dt):
    """One step of the chosen method (lasagne.updates.sgd / adam) in dtype ``dt``; a_t formed in float64."""
    if method == "sgd":
        return theta - lr * grad, m, v
    a_t = lr * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
    one = torch.ones((), dtype=dt)
    m = BETA1 * m + (one - BETA1) * grad
    v = BETA2 * v + (one - BETA2) * grad * grad
    return theta - torch.as_tensor(a_t, dtype=dt) * m / (torch.sqrt(v) + EPS), m, v


def restated_update(cfg, st, pool, rows, dt, swap_order=False, no_mean=False, decay_biases=False, drop_term=False):
    """One update at pool rows ``rows`` [B] in dtype ``dt``.  Returns (new state, dict(q, y, qf_loss, surr)).  The
    keyword variants are the mistakes the power checks must be able to see: the policy step before the Q step, a loss
    summed instead of averaged, decay on the biases too, the terminal mask dropped."""
    D, A, hs = cfg["D"], cfg["A"], cfg["hs"]
    c = lambda x: x.to(dt)
    rows = torch.as_tensor(rows, dtype=torch.int64)
    s, a, r, term, s2 = (c(pool[k][rows]) for k in ("obs", "act", "rew", "term", "next_obs"))
    pi, q, tpi, tq = c(st["pi"]), c(st["q"]), c(st["tpi"]), c(st["tq"])
    wm_q, wm_pi = c(weight_mask(D, A, hs, A, 1)), c(weight_mask(D, A, hs, 0, A))
    if decay_biases:
        wm_q, wm_pi = torch.ones_like(wm_q), torch.ones_like(wm_pi)
    red = (lambda x: x.sum()) if no_mean else (lambda x: x.mean())
    with torch.no_grad():
        q2 = q_forward(tq, s2, pi_forward(tpi, s2, cfg), cfg)
        y = r + (torch.ones_like(term) if drop_term else 1.0 - term) * cfg["discount"] * q2
    new = dict(st)
    new["t_q"], new["t_pi"] = st["t_q"] + 1, st["t_pi"] + 1
    out = {}

    def q_step(q_now):
        qv = q_now.detach().clone().requires_grad_(True)
        qval = q_forward(qv, s, a, cfg)
        loss = red((y - qval) ** 2)
        reg = loss + 0.5 * cfg["qf_wd"] * ((qv * wm_q) ** 2).sum()
        g = torch.autograd.grad(reg, qv)[0]
        out["q"], out["y"], out["qf_loss"] = qval.detach().double(), y.double(), loss.detach().double()
        return _step(q_now, g, c(st["m_q"]), c(st["v_q"]), new["t_q"], cfg["qf_method"], cfg["qf_lr"], dt)

    def pi_step(pi_now, q_used):
        pv = pi_now.detach().clone().requires_grad_(True)
        surr = -red(q_forward(q_used.detach(), s, pi_forward(pv, s, cfg), cfg))
        reg = surr + 0.5 * cfg["pi_wd"] * ((pv * wm_pi) ** 2).sum()
        g = torch.autograd.grad(reg, pv)[0]
        out["surr"] = surr.detach().double()
        return _step(pi_now, g, c(st["m_pi"]), c(st["v_pi"]), new["t_pi"], cfg["pi_method"], cfg["pi_lr"], dt)

    if swap_order:
        pi_new, m_pi, v_pi = pi_step(pi, q)
        q_new, m_q, v_q = q_step(q)
    else:
        q_new, m_q, v_q = q_step(q)
        pi_new, m_pi, v_pi = pi_step(pi, q_new)
    tau = cfg["tau"]
    new.update(pi=pi_new.detach(), q=q_new.detach(), m_pi=m_pi.detach(), v_pi=v_pi.detach(), m_q=m_q.detach(),
               v_q=v_q.detach(), tpi=(tpi * (1.0 - tau) + pi_new.detach() * tau), tq=(tq * (1.0 - tau) + q_new.detach() * tau))
    return new, out


def run_updates(cfg, st, pool, indices, dt, **variant):
    """``indices`` [K, B] -> (state after K updates, list of per-update outputs)."""
    outs = []
    for k in range(indices.shape[0]):
        st, o = restated_update(cfg, st, pool, indices[k], dt, **variant)
        outs.append(o)
    return st, outs


def movement_blocks(cfg):
    """Blocks of the concatenated movement vector [pi | q | tpi | tq]."""
    D, A, hs = cfg["D"], cfg["A"], cfg["hs"]
    res, off = [], 0
    for prefix, merge, out in (("pi.", 0, A), ("q.", A, 1), ("targ_pi.", 0, A), ("targ_q.", A, 1)):
        bl = blocks(D, A, hs, merge, out, prefix)
        res += [(n, off + b, off + e) for n, b, e in bl]
        off += bl[-1][2]
    return res


def movement(before, after):
    """theta_after - theta_before of the four vectors, concatenated, float64."""
    return torch.cat([after[k].double() - before[k].double() for k in ("pi", "q", "tpi", "tq")])


def rel_errors(got, ref64, blocks_):
    return {name: float((got[b:e] - ref64[b:e]).norm()) / float(ref64[b:e].norm()) for name, b, e in blocks_}


def within_blocks(name, got, ref64, ref32, blocks_):
    """e_k(block) <= ALLOW max(e_32(block), FLOOR) on every block's own norm; one line per block, every block is looked
    at before the first failure is raised."""
    bad = []
    for bname, b, e in blocks_:
        r = ref64[b:e]
        n64 = float(r.norm())
        assert n64 > 0 and np.isfinite(n64), (name, bname, n64)            # nothing is compared vacuously
        e_k = float((got[b:e] - r).norm()) / n64
        e_32 = float((ref32[b:e] - r).norm()) / n64
        print("%s [%s]: kernel %.3e, float32 restatement %.3e, ratio to the floored yardstick %.2f" % (
            name, bname, e_k, e_32, e_k / max(e_32, FLOOR)))
        if not e_k <= ALLOW * max(e_32, FLOOR):
            bad.append(bname)
    assert not bad, (name, bad)


def draw_rows(seed, counter, B, size, top, cap, skip, attempts=32):
    """The batch rows of update ``counter`` by the rule of rl_ddpg_update: slot b takes word 0 of Philox4x32-10 at
    counters (attempt, b, c_lo, c_hi), key seed; logical index (word * size) >> 32; physical row
    (top - size + index) mod cap; a row with skip = 1 is redrawn with the next attempt; after ``attempts`` the walk goes
    forward (mod size) to the first kept row (the last drawn row if every row is skipped)."""
    from oracle.host_env import philox
    skip = np.asarray(skip)
    rows = np.zeros(B, dtype=np.int64)
    for b in range(B):
        words = philox(0, b, counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF,
                       (seed >> 32) & 0xFFFFFFFF, attempts)[:, 0].astype(np.uint64)
        index = None
        for w in words:
            index = int((int(w) * size) >> 32)
            row = (top - size + index) % cap
            if skip[row] == 0:
                break
        else:
            row = (top - size + index) % cap
            for step in range(1, size + 1):
                cand = (top - size + (index + step) % size) % cap
                if skip[cand] == 0:
                    row = cand
                    break
        rows[b] = row
    return rows


# ---- the inputs the host and the GPU tests share (built once, never written to) --------------------------------------
# Rates at which one step moves a block by 1e-3 .. 1e-1 of its norm: the parameters are stored in float32, so a movement
# is known to 2^-24 |theta| at best, and at the reference's rates (1e-3, 1e-4, tau 1e-3) that rounding would be the
# whole yardstick -- several per cent of the policy's movement -- and would hide a wrong factor in a gradient.
BIG_STEPS = dict(qf_lr=0.05, pi_lr=0.5, tau=0.5)
_CASES = {}


def _case(kind, shape, **cfg_kw):
    key = (kind, shape)
    if key not in _CASES:
        D, A, hs, hact, B = shape
        cfg = make_cfg(D, A, hs, hact, B, **cfg_kw)
        st, pool = make_state(cfg, seed=len(_CASES)), make_pool(cfg, seed=100 + len(_CASES))
        idx = make_indices(cfg, 2, seed=200 + len(_CASES))
        pool["term"][idx[0, 0].long()] = 1.0          # batch 0 holds a terminal row ...
        if not (pool["term"][idx[1].long()] == 0).any():
            pool["term"][idx[1, 0].long()] = 0.0      # ... and batch 1 one that is not (B = 1)
        _CASES[key] = (cfg, st, pool, idx)
    return _CASES[key]


def sgd_case(shape):
    """SGD on both nets: the movement is -lr x gradient, so a scale error in a gradient is a scale error here."""
    return _case("sgd", shape, **BIG_STEPS)


def order_case(shape):
    """SGD with a large Q rate: the Q parameters the policy step sees depend visibly on whether the Q step ran."""
    return _case("order", shape, **dict(BIG_STEPS, qf_lr=0.3))


def decay_case(shape):
    return _case("decay", shape, qf_wd=0.1, pi_wd=0.1, **BIG_STEPS)


def adam_case(shape):
    return _case("adam", shape, qf_method="adam", pi_method="adam", qf_wd=0.01, pi_wd=0.01)
