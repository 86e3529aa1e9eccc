"""Host side of the recurrent population rollout (rl_rollout_population_gru): the rows ``GRUPolicyBase.pack_rows`` hands the
kernel, and the entry point's declaration.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(do, da, hidden, include_action, seed=0):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.spaces import Box
    np.random.seed(seed)
    return GaussianGRUPolicy(EnvSpec(Box(-np.ones(do), np.ones(do)), Box(-np.ones(da), np.ones(da))),
                             hidden_sizes=(hidden,), state_include_action=include_action)


@pytest.mark.parametrize("include_action", [True, False])
@pytest.mark.parametrize("hidden", [20, 32, 50, 64])
def test_pack_rows_is_pad_index_row_by_row(hidden, include_action):
    do, da, n_cand = 13, 2, 5
    pol = _policy(do, da, hidden, include_action)
    P = pol.get_param_values().size
    xs = np.random.RandomState(3).randn(n_cand, P).astype(np.float32)
    assert np.all(xs != 0)
    rows = pol.pack_rows(torch.as_tensor(xs, device=pol.flat_params.device))
    assert rows.dtype == torch.float32 and rows.device == pol.flat_params.device
    rows = rows.cpu().numpy()
    # P_pad: GruLayout<H, Da>(DI).total + Da (csrc/gru_cell.h) at the kernel's width
    H = pol.kernel_hidden
    assert H == (32 if hidden <= 32 else 64)
    di = do + (da if include_action else 0)
    total = H + 3 * (di * H + H * H + H) + H * da + da
    idx, size = pol.pad_index()
    assert size == total + da and rows.shape == (n_cand, size)
    padded = np.ones(size, dtype=bool)
    padded[idx] = False
    assert int(padded.sum()) == size - P
    for c in range(n_cand):
        want = np.zeros(size, dtype=np.float32)
        want[idx] = xs[c]
        assert np.array_equal(rows[c], want), c
        assert np.all(rows[c][padded] == 0)
    # what rollout_layout() would hold after set_param_values(xs[c]): the same index copy (its buffer needs a HIP device)
    pol.set_param_values(xs[2])
    lay = np.zeros(size, dtype=np.float32)
    lay[idx] = pol.get_param_values().astype(np.float32)
    assert np.array_equal(rows[2], lay)


def test_entry_point_is_declared_and_bound():
    from rllab_amd import _lib
    text = open(os.path.join(ROOT, "include", "rllab_amd.h")).read()
    assert re.search(r"int rl_rollout_population_gru\(const rl_population_gru_args\* \w+, void\* \w+\);", text)
    assert "rl_rollout_population_gru" in _lib.SYMBOLS
    assert list(_lib.lib.rl_rollout_population_gru.argtypes) == [ctypes.POINTER(_lib.PopulationGruArgs), ctypes.c_void_p]
    assert _lib.lib.rl_abi_version() == 14
    # the struct: rl_population_args with include_action in the place of layer_activations
    body = lambda name: re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text,
                                                          flags=re.S).group(1), flags=re.S)
    fields = lambda name: [d.strip().split()[-1].lstrip("*") for d in body(name).split(";") if d.strip()]
    want = ["include_action" if f == "layer_activations" else f for f in fields("rl_population_args")]
    assert fields("rl_population_gru_args") == want == [f for f, _ in _lib.PopulationGruArgs._fields_]
    assert ctypes.sizeof(_lib.PopulationGruArgs) == ctypes.sizeof(_lib.PopulationArgs)
    # argument errors come back as status codes, nothing is launched
    assert _lib.lib.rl_rollout_population_gru(None, None) == -1
    assert b"rl_rollout_population_gru" in _lib.lib.rl_last_error()
    assert _lib.lib.rl_rollout_population_gru(ctypes.byref(_lib.PopulationGruArgs()), None) == -1


def test_refusal_function_takes_a_gru_policy():
    """population_why_unsupported stays one function for both algorithms; what it says of a GaussianGRUPolicy off the GPU
    is that policy's own sentence."""
    from rllab_amd.algos import cem, cma_es
    from rllab_amd.envs.box2d.cartpole_env import CartpoleEnv
    from rllab_amd.envs.normalized_env import normalize
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    assert cma_es.population_why_unsupported is cem.population_why_unsupported
    env = normalize(CartpoleEnv())
    wide = GaussianGRUPolicy(env_spec=env.spec, hidden_sizes=(100,))
    assert "hidden_sizes=(100,)" in cem.population_why_unsupported(env, wide)
    assert cem.population_why_unsupported(env, wide) == wide.why_no_rollout_kernel()
    pol = GaussianGRUPolicy(env_spec=env.spec, hidden_sizes=(32,))
    assert cem.population_why_unsupported(env, pol) == pol.why_no_rollout_kernel()
    assert "normalize_obs" in cem.population_why_unsupported(normalize(CartpoleEnv(), normalize_obs=True), pol)
    assert "plot=True" in cem.population_why_unsupported(env, pol, plot=True)
    # CMA-ES: 13 570 parameters of a 64-unit GRU on Cartpole are past MAX_PARAMS, 3 714 of a 32-unit one are not
    big = GaussianGRUPolicy(env_spec=env.spec, hidden_sizes=(64,))
    assert big.get_param_values().size == 13570 and pol.get_param_values().size == 3714
    assert "13570 parameters" in cma_es.CMAES(env=env, policy=big).why_unsupported()
    assert "more than 8192" not in (cma_es.CMAES(env=env, policy=pol).why_unsupported() or "")
