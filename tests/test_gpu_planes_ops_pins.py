"""Every output bit of the networks-on-planes update passes (FusedAdaptiveStdOps: two networks + the Gaussian head,
FusedCategoricalOps: one network + the categorical head), pinned: tests/golden/planes_ops.json holds, per case and per
output, a SHA-256 of the bytes, recorded by tools/make_golden_planes_ops.py with the code of the commit its header names.
The parity tests of these classes (tests/test_gpu_adaptive_std.py, tests/test_gpu_categorical.py) hold them to 2e-5 of
float64 autograd; a changed argument, a changed launch order or a parameter copy that was not refreshed can pass those.
This one does not: a digest that differs is a defect of the change, never a reason to record again.

The recorder runs every case in two processes; an output whose digests differ between them is recorded as unstable, with
its values, and compared here at the bar the parity test of the same quantity uses (``PARITY``), nothing wider.

Shapes, the smallest at which padding, the identity layer and both kernel families can go wrong: (4, 1) with a (32, 32) mean
net and an (8,) std net -- one wavefront per tile, and a padded one-hidden-layer net with its constant identity layer;
(5, 2) with (32, 32) / (16, 16) -- the cooperative kernels ((5, 2) is not a pair the one-wavefront kernels are instantiated
for); 9 one-hot states / 4 actions with (8,) and (32, 32).  Each at B = 96 (three whole tiles) and B = 70 (a ragged tail),
about a fifth of the weights zero."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planes_ops.json")
CASES = {}
for _B in (96, 70):
    CASES["adaptive_4_1_h32x32_s8_B%d" % _B] = ("adaptive", dict(do=4, da=1, hm=(32, 32), hs=(8,)), _B)
    CASES["adaptive_5_2_h32x32_s16x16_B%d" % _B] = ("adaptive", dict(do=5, da=2, hm=(32, 32), hs=(16, 16)), _B)
    CASES["categorical_9_4_h8_B%d" % _B] = ("categorical", dict(do=9, da=4, hidden=(8,)), _B)
    CASES["categorical_9_4_h32x32_B%d" % _B] = ("categorical", dict(do=9, da=4, hidden=(32, 32)), _B)
# relative bar of tests/test_gpu_adaptive_std.py / tests/test_gpu_categorical.py for the same quantity, and the floor of its scale
PARITY = dict(loss_stats=(2e-5, 1e-2), loss_stats_of_grad_pass=(2e-5, 1e-2), loss_grad=(2e-5, 1e-3), fvp=(5e-5, 0.0),
              cg_x=(1e-4, 0.0), cg_xHx=(1e-4, 0.0), value=(2e-5, 1.0), value_grad=(2e-5, 1e-3))


def _inputs(kind, pol, B):
    from tests.test_gpu_adaptive_std import _inputs as gaussian_inputs
    from tests.test_gpu_categorical import _inputs as categorical_inputs
    inp = list(gaussian_inputs(pol, B) if kind == "adaptive" else categorical_inputs(pol, B))
    if kind == "categorical":                                              # one-hot states, as GridWorld's batches have
        idx = np.random.RandomState(4).randint(0, pol.obs_dim, size=B)
        inp[0] = torch.as_tensor(np.eye(pol.obs_dim, dtype=np.float32)[idx].T.copy(), device=inp[0].device)
    w = torch.as_tensor((np.random.RandomState(5).rand(B) >= 0.2).astype(np.float32), device=inp[0].device)
    w[0] = 1.0
    assert 0.1 * B <= float((w == 0).sum()) <= 0.3 * B
    inp[-2], inp[-1] = w, 1.0 / w.double().sum()
    return tuple(inp)


def run_case(name):
    """{output name: float64 / float32 numpy array} of one case, on the current device."""
    kind, kw, B = CASES[name]
    if kind == "adaptive":
        from tests.test_gpu_adaptive_std import _policy
        pol = _policy(kw["do"], kw["da"], kw["hm"], kw["hs"])
    else:
        from tests.test_gpu_categorical import _policy
        pol = _policy(kw["do"], kw["da"], kw["hidden"])
    ops = pol.fused_ops()
    assert type(ops).__name__ == ("FusedAdaptiveStdOps" if kind == "adaptive" else "FusedCategoricalOps")
    inp = _inputs(kind, pol, B)
    assert ops.accepts(inp)
    out = dict(loss_stats=ops.loss_stats(inp).clone())
    ops.release()
    g = ops.loss_grad(inp, with_loss=True)
    out["loss_grad"] = g.clone()
    out["loss_stats_of_grad_pass"] = ops.loss_stats(inp).clone()          # (the gradient pass's record: no pass of its own)
    v = torch.as_tensor(np.random.RandomState(6).randn(g.numel()), device=g.device)
    out["fvp"] = ops.fvp(inp, v)
    out["cg_x"], out["cg_xHx"] = ops.cg(inp, g, 3, 1e-5)
    val, vg = ops.value_and_grad(inp, penalty=0.5)
    out["value"], out["value_grad"] = np.asarray([val], dtype=np.float64), np.asarray(vg)
    torch.cuda.synchronize()
    return {k: np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t).reshape(-1) for k, t in out.items()}


def digest(a):
    return dict(dtype=str(a.dtype), n=int(a.size), sha256=hashlib.sha256(a.tobytes()).hexdigest())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["parent_commit"]) == 40 and sorted(g["cases"]) == sorted(CASES)
    return g["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_planes_ops_bits(name, golden):
    got, want = run_case(name), golden[name]
    assert sorted(got) == sorted(want) == sorted(PARITY)
    for k in sorted(want):
        if "values" not in want[k]:
            assert digest(got[k]) == want[k], "%s: output %r differs from the recorded pass" % (name, k)
            continue
        ref = np.asarray([float.fromhex(h) for h in want[k]["values"]])    # unstable at the parent: the parity bar
        rel, floor = PARITY[k]
        assert got[k].shape == ref.shape and np.abs(got[k] - ref).max() <= rel * max(floor, np.abs(ref).max()), (name, k)
