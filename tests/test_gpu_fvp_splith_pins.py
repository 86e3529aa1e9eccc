"""Every output bit of the two-way f16 split Fisher-vector product (csrc/policy_splith_kernels.hip, rl_policy_fvp variant 4),
pinned: tests/golden/fvp_splith_pins.json holds, per case, the shape, the dtype and a SHA-256 of the float64 product,
recorded by tools/make_golden_fvp_splith.py with the library of the commit its header names -- the commit BEFORE the
sample-major parts of h0, gz1~ and gz0~ went through an LDS image and ds_read_b64_tr_b16 instead of a product with an
identity on the matrix pipe.  Both transpositions are exact and hand every matrix instruction of the two sample-contracted
products the same operands in the same k positions, so a digest that differs is a wrong address map, a read under a partial
EXEC mask, an image overwritten before it was read -- never a reason to record again.  The parity tests
(tests/test_gpu_fvp_split.py) hold the product to 5e-5 of float64; a transposed read that returns a neighbouring sample's
value at a small magnitude can pass them.

The sample counts are the smallest at which the change can still go wrong: one tile (the other wavefronts of the workgroup
idle), a second workgroup with ONE active wavefront, and, at the capped grid of 256 workgroups, three tiles more than one
per wavefront, so that some wavefronts reuse their LDS region for a second tile.  (21, 6) has two k-blocks of inputs,
(20, 6) runs one wavefront per SIMD; the (64, 64) kernel and the observation operand stayed on the matrix pipe and keep
their cases."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_update_parity as U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fvp_splith_pins.json")

CASES = {}
for _do, _da in ((4, 1), (13, 2), (20, 6), (21, 6)):
    for _B in (32, 32 * 9, 32 * (2048 + 3)):
        CASES["h32_do%d_da%d_B%d" % (_do, _da, _B)] = (_do, _da, 32, _B)
for _do, _da in ((13, 2), (20, 6)):
    for _B in (32, 32 * 5, 32 * (1024 + 3)):
        CASES["h64_do%d_da%d_B%d" % (_do, _da, _B)] = (_do, _da, 64, _B)


def run_case(name):
    """dict(shape, dtype, sha256) of the float64 product of one case, on the current device."""
    do, da, h, B = CASES[name]
    pol = U._policy(do, da, h)
    rng = np.random.RandomState(101 + do + 7 * da + h)
    n = pol.get_param_values().size
    pol.set_param_values(0.3 * rng.randn(n))                      # theta: seeded numpy, whatever the initialiser drew
    direction = torch.as_tensor(rng.randn(n), device="cuda")
    inp = U._inputs(pol, B, seed=3, old_equals_new=True)          # seeded numpy observations; a tenth of the weights zero
    assert B < 64 or float((inp[5] == 0).sum()) > 0
    ops = pol.fused_ops()
    ops.loss_grad(inp, keep_activations=True)                     # fills the activation cache and obs_absmax, as the optimizer does
    assert ops.fvp_variant(inp) == 4                              # the launch below IS the f16 split kernel
    a = np.ascontiguousarray(ops.fvp(inp, direction).cpu().numpy())
    assert a.dtype == np.float64 and np.all(np.isfinite(a)) and np.abs(a).max() > 0
    return dict(shape=list(a.shape), dtype=str(a.dtype), sha256=hashlib.sha256(a.tobytes()).hexdigest())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["parent_commit"]) == 40 and sorted(g["cases"]) == sorted(CASES)
    return g["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fvp_splith_bits(name, golden):
    got = run_case(name)
    assert got == golden[name], "%s: the product differs from the recorded launch" % name
