"""The recurrent categorical update kernels without a GPU: symbols, argument errors, the plan (which maps fit the LDS of a
CU at which width), and the Python side of CategoricalGRUPolicy(bptt_kernels=True) on CPU parameters."""
import ctypes

import numpy as np
import pytest
import torch

NEW = ("rl_gru_categorical_workspace_bytes", "rl_gru_categorical_eval", "rl_gru_categorical_grad",
       "rl_gru_categorical_fvp")
MAPS = {"4x4": 16, "chain": 29, "8x8": 64}            # GridWorldEnv's maps: their number of states


def _batch(**kw):
    """A descriptor whose pointers are non-NULL and never dereferenced: every call below fails before a launch."""
    from rllab_amd import _lib
    a = dict(n_envs=70, horizon=25, n_states=16, n_act=4, hidden=32, include_action=1, inv_count=1.0 / 1750,
             theta=64, state=64, action=64, advantages=64, old_prob=64, start=64, weights=64, workspace=64,
             workspace_bytes=1 << 40)
    a.update(kw)
    return _lib.GruCategoricalBatch(**a)


def _calls(b):
    from rllab_amd import _lib
    lib, p = _lib.lib, ctypes.byref(b)
    return (lib.rl_gru_categorical_eval(p, 64, None), lib.rl_gru_categorical_grad(p, 64, 64, None),
            lib.rl_gru_categorical_fvp(p, 64, 64, None))


def test_symbols_are_exported_and_bound():
    from rllab_amd import _lib
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.rl_gru_categorical_workspace_bytes.restype is ctypes.c_size_t
    assert [f for f, _ in _lib.GruCategoricalBatch._fields_][:6] == ["n_envs", "horizon", "n_states", "n_act", "hidden",
                                                                    "include_action"]


def test_struct_layout_against_the_compiled_header(tmp_path):
    import os
    import subprocess
    from rllab_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include "rllab_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("size %zu\\n", sizeof(rl_gru_categorical_batch));']
    for f, _ in _lib.GruCategoricalBatch._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rl_gru_categorical_batch, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.GruCategoricalBatch)
    for f, _ in _lib.GruCategoricalBatch._fields_:
        assert int(got[f]) == getattr(_lib.GruCategoricalBatch, f).offset, f


def test_argument_errors():
    from rllab_amd import _lib
    lib = _lib.lib
    assert lib.rl_gru_categorical_eval(None, 64, None) == -1 and "null" in lib.rl_last_error().decode()
    assert lib.rl_gru_categorical_grad(None, 64, 64, None) == -1 and lib.rl_gru_categorical_fvp(None, 64, 64, None) == -1
    for kw in (dict(n_envs=0), dict(horizon=0), dict(n_envs=1 << 16, horizon=1 << 15), dict(n_states=0), dict(n_act=3),
               dict(n_act=5), dict(include_action=2), dict(inv_count=0.0), dict(theta=None), dict(state=None),
               dict(action=None), dict(advantages=None), dict(old_prob=None), dict(start=None), dict(weights=None),
               dict(workspace=None), dict(workspace_bytes=16)):
        assert _calls(_batch(**kw)) == (-1, -1, -1), kw
    p = ctypes.byref(_batch())
    assert lib.rl_gru_categorical_eval(p, None, None) == -1                      # the outputs
    assert lib.rl_gru_categorical_grad(p, None, 64, None) == -1 and lib.rl_gru_categorical_grad(p, 64, None, None) == -1
    assert lib.rl_gru_categorical_fvp(p, None, 64, None) == -1 and lib.rl_gru_categorical_fvp(p, 64, None, None) == -1
    assert "workspace of 16 bytes" in (_calls(_batch(workspace_bytes=16)) and lib.rl_last_error().decode())


def _lds_bytes(S, H, inc=1):
    """The issue's arithmetic: the larger of 2 P + 3 tiles (tangent sweep) and P + 5 tiles (backward sweep)."""
    DI = S + 4 * inc
    P = H + 3 * (DI * H + H * H + H) + 4 * H + 4
    return 4 * max(2 * P + 3 * H * 64, P + 5 * H * 64)


def test_the_plan():
    from rllab_amd import _lib
    lib = _lib.lib
    ws = lib.rl_gru_categorical_workspace_bytes
    for name, S in MAPS.items():
        assert _lds_bytes(S, 32) <= 160 * 1024
        for inc in (0, 1):
            assert ws(4096, 100, S, 32, inc) > 0, (name, inc)
    assert (_lds_bytes(16, 32), _lds_bytes(29, 32), _lds_bytes(64, 32)) == (66592, 76576, 103456)
    assert ws(1, 1, 16, 32, 1) > 0
    # the planes dominate: h and the four cotangent planes [H][B], the logits' [4][B]
    B = 4096 * 100
    assert ws(4096, 100, 16, 32, 1) >= (5 * 32 + 4) * B * 4
    assert ws(4096, 100, 16, 32, 1) > ws(2048, 100, 16, 32, 1)
    # 4x4 at 64 units: over the LDS of a CU, the byte count is in the message; no width in between is built
    assert ws(70, 25, 16, 64, 1) == 0
    msg = lib.rl_last_error().decode()
    assert "bytes of LDS" in msg and int(msg.split(":")[1].split()[0]) == _lds_bytes(16, 64) > 160 * 1024
    assert _calls(_batch(hidden=64)) == (-2, -2, -2) and "bytes of LDS" in lib.rl_last_error().decode()
    for hidden in (48, 128, 0):
        assert ws(70, 25, 16, hidden, 1) == 0 and "hidden = %d" % hidden in lib.rl_last_error().decode()
        assert _calls(_batch(hidden=hidden)) == (-2, -2, -2)
    # a map far too large: refused by its byte count, not wrapped into an int
    assert ws(70, 25, 1 << 30, 32, 1) == 0 and "bytes of LDS" in lib.rl_last_error().decode()
    for args in ((0, 25, 16, 32, 1), (70, 0, 16, 32, 1), (1 << 16, 1 << 15, 16, 32, 1), (70, 25, 0, 32, 1)):
        assert ws(*args) == 0, args


def _spec(S=16):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Discrete
    return EnvSpec(Discrete(S), Discrete(4))


def test_the_default_policy_is_as_it_was():
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    pol = CategoricalGRUPolicy(_spec())
    assert pol.bptt_kernels is False and pol.fused_ops() is None
    assert pol.why_no_kernel_layout() == "recurrent policy (no BPTT kernels)"
    with pytest.raises(TypeError):
        CategoricalGRUPolicy(_spec(), bptt_kernel=True)


def test_the_option_on_cpu_parameters_names_the_device():
    import pickle
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    pol = CategoricalGRUPolicy(_spec(), bptt_kernels=True)
    assert pol.bptt_kernels is True
    if not pol.flat_params.is_cuda:
        assert pol.why_no_kernel_layout() == "the parameters are not float32 on a HIP device"
        assert pol.fused_ops() is None
    pol.flat_params = pol.flat_params.detach().cpu().double()
    assert pol.why_no_kernel_layout() == "the parameters are not float32 on a HIP device" and pol.fused_ops() is None
    assert pickle.loads(pickle.dumps(pol)).bptt_kernels is True                  # a Serializable clone keeps the option
    # what keeps a policy off the kernels is said ahead of the device
    wide = CategoricalGRUPolicy(_spec(), hidden_dim=100, bptt_kernels=True)
    assert wide.why_no_kernel_layout() == "hidden_dim=100: the recurrent update kernels run 1 .. 64 hidden units"


def test_the_ops_class_on_cpu_parameters():
    """The ops class on CPU parameters: the padded layout round trip, the frozen entries, and ``accepts`` refusing planes
    that are not on the device -- once per tuple in the log."""
    from rllab_amd.misc import logger
    from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
    from rllab_amd.policies.fused_categorical_gru_ops import FusedCategoricalGRUOps
    from rllab_amd.policies.fused_gru_ops import FusedGRUOps, RecurrentOpsBase
    assert issubclass(FusedCategoricalGRUOps, RecurrentOpsBase) and issubclass(FusedGRUOps, RecurrentOpsBase)
    pol = CategoricalGRUPolicy(_spec(), hidden_dim=20, bptt_kernels=True)
    pol.flat_params = pol.flat_params.detach().cpu()
    ops = FusedCategoricalGRUOps(pol)
    idx, size = pol.pad_index()
    assert ops.n_flat == pol.flat_params.numel() and ops.n_kernel == size == 32 + 3 * (20 * 32 + 32 * 32 + 32) + 32 * 4 + 4
    v = torch.as_tensor(np.random.RandomState(0).randn(ops.n_flat) + 3.0)
    k = ops.scatter(v)
    assert k.dtype == torch.float32 and k.numel() == size and torch.equal(ops.gather(k), v.float())
    assert ops.frozen.tolist() == list(range(20))
    T, N = 3, 5
    inputs = (torch.zeros(16, T, N), torch.zeros(4, T, N), torch.zeros(T, N), torch.zeros(4, T, N),
              torch.ones(T, N, dtype=torch.bool), torch.ones(T, N), torch.tensor(1.0 / (T * N), dtype=torch.float64))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        txt = d + "/log.txt"
        logger.add_text_output(txt)
        logger.set_quiet(True)
        try:
            assert not ops.accepts(inputs) and not ops.accepts(inputs)
        finally:
            logger.remove_text_output(txt)
            logger.set_quiet(False)
        assert open(txt).read().count("update path: torch autograd for this batch") == 1
