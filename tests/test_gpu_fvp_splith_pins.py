"""Every output bit of the split-operand Fisher-vector products, pinned: per case the shape, the dtype and a SHA-256 of the
float64 product, recorded by tools/make_golden_fvp_splith.py with the library of the commit the file's header names.

tests/golden/fvp_splith_pins.json -- the two-way f16 split (csrc/policy_splith_kernels.hip, rl_policy_fvp variant 4), recorded
at the commit BEFORE the sample-major parts of h0, gz1~ and gz0~ went through an LDS image and ds_read_b64_tr_b16 instead of
a product with an identity on the matrix pipe.  Both transpositions are exact and hand every matrix instruction of the two
sample-contracted products the same operands in the same k positions, so a digest that differs is a wrong address map, a read
under a partial EXEC mask, an image overwritten before it was read -- never a reason to record again.

tests/golden/fvp_split_pins.json -- the three-way bf16 split (csrc/policy_split_kernels.hip, variant 1), its 16-sample-tile
form (csrc/policy_split16_kernels.hip, variant 3, three and four wavefronts per SIMD) and the cooperative kernel
(csrc/policy_csplit_kernels.hip, variant 2), recorded at the commit BEFORE the code these files share moved into
csrc/fvp_split_common.h and their settled build-time switches went: a move changes no instruction, so no bit.

The parity tests (tests/test_gpu_fvp_split.py, tests/test_gpu_csplit.py) hold the products to 5e-5 of float64; a transposed
read that returns a neighbouring sample's value at a small magnitude can pass them.

The sample counts are the smallest at which a wrong address or fold can still show: one tile (the other wavefronts of the
workgroup idle), a second workgroup with ONE active wavefront, and, at the capped grid, three tiles more than one per
wavefront, so that some wavefronts reuse their LDS region for a second tile.  (21, 6) has two k-blocks of inputs, (20, 6) runs
one wavefront per SIMD."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_update_parity as U
from tests.test_gpu_wide_nets import _policy as _wide_policy

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = {"splith": os.path.join(GOLDEN_DIR, "fvp_splith_pins.json"), "split": os.path.join(GOLDEN_DIR, "fvp_split_pins.json")}
FVP_SWITCHES = ("RLLAB_FVP_SPLIT", "RLLAB_FVP_SPLIT_WPS")


def _counts(waves, tile=32, grid_cap=256):
    """Sample counts of a kernel that hands one ``tile``-sample tile to each of the ``waves`` wavefronts of a workgroup, on at
    most ``grid_cap`` workgroups; whole 32-sample tiles (a 16-sample-tile count is rounded up to an even number of tiles)."""
    return [32 * ((n * tile + 31) // 32) for n in (1, waves + 1, grid_cap * waves + 3)]


# name -> (file, variant rl_policy_fvp_variant must report, {switch: value}, obs_dim, act_dim, hidden, n_samples)
CASES = {}
for _do, _da in ((4, 1), (13, 2), (20, 6), (21, 6)):
    for _B in (32, 32 * 9, 32 * (2048 + 3)):
        CASES["h32_do%d_da%d_B%d" % (_do, _da, _B)] = ("splith", 4, {}, _do, _da, 32, _B)
for _do, _da in ((13, 2), (20, 6)):
    for _B in (32, 32 * 5, 32 * (1024 + 3)):
        CASES["h64_do%d_da%d_B%d" % (_do, _da, _B)] = ("splith", 4, {}, _do, _da, 64, _B)
# fvp_split_kernel: two wavefronts per SIMD (eight per workgroup), heads wider than two outputs one (four)
for _do, _da in ((4, 1), (13, 2), (20, 6), (21, 6)):
    for _B in _counts(8 if _da <= 2 else 4):
        CASES["b32_do%d_da%d_B%d" % (_do, _da, _B)] = ("split", 1, {"RLLAB_FVP_SPLIT": "5"}, _do, _da, 32, _B)
# fvp_split64_kernel: one wavefront per SIMD
for _do, _da in ((13, 2), (20, 6)):
    for _B in _counts(4):
        CASES["b64_do%d_da%d_B%d" % (_do, _da, _B)] = ("split", 1, {"RLLAB_FVP_SPLIT": "5"}, _do, _da, 64, _B)
# fvp_split16_kernel: 16-sample tiles, three wavefronts per SIMD (twelve per workgroup), or four on request
for _wps in (3, 4):
    for _do, _da in ((4, 1), (13, 2)):
        for _B in _counts(4 * _wps, tile=16):
            _env = {"RLLAB_FVP_SPLIT": "3"}
            if _wps == 4:
                _env["RLLAB_FVP_SPLIT_WPS"] = "4"
            CASES["t16w%d_do%d_da%d_B%d" % (_wps, _do, _da, _B)] = ("split", 3, _env, _do, _da, 32, _B)
# the cooperative kernel: ONE tile per workgroup (two or four wavefronts share it), its grid capped at two workgroups per CU
# (64-unit layers, LDS permitting) or one (a 128-unit layer) -- CS_MAX_GRID = 512 is at or past the cap of either
for _hidden in ((64, 64), (128, 128)):
    for _B in (32, 32 * 2, 32 * (512 + 3)):
        CASES["c%d_do20_da6_B%d" % (_hidden[0], _B)] = ("split", 2, {"RLLAB_FVP_SPLIT": "2"}, 20, 6, _hidden, _B)


def run_case(name):
    """dict(shape, dtype, sha256) of the float64 product of one case, on the current device."""
    _, variant, env, do, da, h, B = CASES[name]
    if isinstance(h, tuple):                                      # (the 64-unit pair is a policy of the narrow family)
        pol, h = (U._policy(do, da, 64) if h == (64, 64) else _wide_policy(do, da, h)), h[0]
    else:
        pol = U._policy(do, da, h)
    rng = np.random.RandomState(101 + do + 7 * da + h)
    n = pol.get_param_values().size
    pol.set_param_values(0.3 * rng.randn(n))                      # theta: seeded numpy, whatever the initialiser drew
    ops = pol.fused_ops()
    direction = torch.as_tensor(rng.randn(n), device="cuda")
    inp = U._inputs(pol, B, seed=3, old_equals_new=True)          # seeded numpy observations; a tenth of the weights zero
    assert B < 64 or float((inp[5] == 0).sum()) > 0
    saved = {k: os.environ.pop(k, None) for k in FVP_SWITCHES}
    try:
        os.environ.update(env)
        ops.loss_grad(inp, keep_activations=True)                 # fills the activation cache and obs_absmax, as the optimizer does
        assert ops.fvp_variant(inp) == variant                    # the launch below IS that kernel
        a = np.ascontiguousarray(ops.fvp(inp, direction).cpu().numpy())
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert a.dtype == np.float64 and np.all(np.isfinite(a)) and np.abs(a).max() > 0
    return dict(shape=list(a.shape), dtype=str(a.dtype), sha256=hashlib.sha256(a.tobytes()).hexdigest())


@pytest.fixture(scope="module")
def golden():
    cases = {}
    for which, path in GOLDEN.items():
        with open(path) as f:
            g = json.load(f)
        assert len(g["parent_commit"]) == 40 and not set(g["cases"]) & set(cases)
        assert all(CASES[name][0] == which for name in g["cases"])
        cases.update(g["cases"])
    assert sorted(cases) == sorted(CASES)
    return cases


@pytest.mark.parametrize("name", sorted(CASES))
def test_fvp_splith_bits(name, golden):
    got = run_case(name)
    assert got == golden[name], "%s: the product differs from the recorded launch" % name
