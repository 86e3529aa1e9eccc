"""The recurrent update kernels without a GPU: symbols, argument errors, the shapes that are built, and the Python side of
GaussianGRUPolicy(bptt_kernels=True) on CPU parameters."""
import ctypes

import numpy as np
import torch

NEW = ("rl_gru_workspace_bytes", "rl_gru_gaussian_eval", "rl_gru_gaussian_grad", "rl_gru_gaussian_fvp")


def _batch(**kw):
    """A descriptor whose pointers are non-NULL and never dereferenced: every call below fails before a launch."""
    from rllab_amd import _lib
    a = dict(n_envs=70, horizon=25, obs_dim=4, act_dim=1, hidden=32, include_action=1, inv_count=1.0 / 1750,
             theta=64, obs=64, actions=64, advantages=64, old_means=64, old_log_std=64, start=64, weights=64,
             workspace=64, workspace_bytes=1 << 40)
    a.update(kw)
    return _lib.GruBatch(**a)


def _calls(b):
    from rllab_amd import _lib
    lib, p = _lib.lib, ctypes.byref(b)
    return (lib.rl_gru_gaussian_eval(p, 64, None), lib.rl_gru_gaussian_grad(p, 64, 64, None),
            lib.rl_gru_gaussian_fvp(p, 64, 64, None))


def test_symbols_are_exported_and_bound():
    from rllab_amd import _lib
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.rl_gru_workspace_bytes.restype is ctypes.c_size_t
    assert [f for f, _ in _lib.GruBatch._fields_][:6] == ["n_envs", "horizon", "obs_dim", "act_dim", "hidden",
                                                         "include_action"]


def test_struct_layout_against_the_compiled_header(tmp_path):
    import os
    import subprocess
    from rllab_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include "rllab_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("size %zu\\n", sizeof(rl_gru_batch));']
    for f, _ in _lib.GruBatch._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rl_gru_batch, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.GruBatch)
    for f, _ in _lib.GruBatch._fields_:
        assert int(got[f]) == getattr(_lib.GruBatch, f).offset, f


def test_argument_errors():
    from rllab_amd import _lib
    lib = _lib.lib
    assert lib.rl_gru_gaussian_eval(None, 64, None) == -1 and "null" in lib.rl_last_error().decode()
    assert lib.rl_gru_gaussian_grad(None, 64, 64, None) == -1 and lib.rl_gru_gaussian_fvp(None, 64, 64, None) == -1
    for kw in (dict(n_envs=0), dict(horizon=0), dict(n_envs=1 << 16, horizon=1 << 15), dict(obs_dim=0), dict(act_dim=-1),
               dict(include_action=2), dict(inv_count=0.0), dict(theta=None), dict(obs=None), dict(actions=None),
               dict(advantages=None), dict(old_means=None), dict(old_log_std=None), dict(start=None), dict(weights=None),
               dict(workspace=None), dict(workspace_bytes=16)):
        assert _calls(_batch(**kw)) == (-1, -1, -1), kw
    p = ctypes.byref(_batch())
    assert lib.rl_gru_gaussian_eval(p, None, None) == -1                      # the outputs
    assert lib.rl_gru_gaussian_grad(p, None, 64, None) == -1 and lib.rl_gru_gaussian_grad(p, 64, None, None) == -1
    assert lib.rl_gru_gaussian_fvp(p, None, 64, None) == -1 and lib.rl_gru_gaussian_fvp(p, 64, None, None) == -1
    assert "workspace of 16 bytes" in (_calls(_batch(workspace_bytes=16)) and lib.rl_last_error().decode())


def test_unbuilt_widths_and_shapes_are_refused():
    from rllab_amd import _lib
    lib = _lib.lib
    for hidden in (48, 128, 0):
        assert _calls(_batch(hidden=hidden)) == (-2, -2, -2)
        assert "hidden = %d" % hidden in lib.rl_last_error().decode()
        assert lib.rl_gru_workspace_bytes(70, 25, 4, 1, hidden, 1) == 0
    assert _calls(_batch(obs_dim=5)) == (-2, -2, -2) and "obs_dim 5 / act_dim 1" in lib.rl_last_error().decode()
    # over the LDS of a CU: the byte count is in the message
    assert _calls(_batch(obs_dim=20, act_dim=6, hidden=64)) == (-2, -2, -2)
    msg = lib.rl_last_error().decode()
    assert "bytes of LDS" in msg and int(msg.split(":")[1].split()[0]) > 160 * 1024


def test_workspace_bytes():
    from rllab_amd import _lib
    ws = _lib.lib.rl_gru_workspace_bytes
    # Cartpole and DoublePendulum at 32 and 64 units, Swimmer and HalfCheetah at 32
    for do, da, H in ((4, 1, 32), (4, 1, 64), (6, 1, 32), (6, 1, 64), (13, 2, 32), (20, 6, 32)):
        for inc in (0, 1):
            assert ws(4096, 100, do, da, H, inc) > 0, (do, da, H, inc)
    assert ws(1, 1, 4, 1, 32, 1) > 0
    # the planes dominate: h and the four cotangent planes [H][B], the mean's [Da][B]
    B = 4096 * 100
    assert ws(4096, 100, 4, 1, 32, 1) >= (5 * 32 + 1) * B * 4
    assert ws(4096, 100, 4, 1, 64, 1) > ws(4096, 100, 4, 1, 32, 1) > ws(2048, 100, 4, 1, 32, 1)
    for args in ((70, 25, 4, 1, 48, 1), (70, 25, 21, 6, 32, 1), (70, 25, 20, 6, 64, 1), (0, 25, 4, 1, 32, 1),
                 (70, 0, 4, 1, 32, 1), (1 << 16, 1 << 15, 4, 1, 32, 1)):
        assert ws(*args) == 0, args


def _spec(do=4, da=1):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Box
    return EnvSpec(Box(-np.ones(do), np.ones(do)), Box(-np.ones(da), np.ones(da)))


def test_the_option_on_cpu_parameters_names_the_device():
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    pol = GaussianGRUPolicy(_spec(), bptt_kernels=True)
    if not pol.flat_params.is_cuda:
        assert pol.why_no_kernel_layout() == "the parameters are not float32 on a HIP device"
        assert pol.fused_ops() is None
    pol.flat_params = pol.flat_params.detach().cpu().double()
    assert pol.why_no_kernel_layout() == "the parameters are not float32 on a HIP device" and pol.fused_ops() is None
    import pickle
    assert pickle.loads(pickle.dumps(pol)).bptt_kernels is True


def test_the_default_policy_is_as_it_was():
    import pytest
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    pol = GaussianGRUPolicy(_spec())
    assert pol.bptt_kernels is False and pol.fused_ops() is None
    assert pol.why_no_kernel_layout() == "recurrent policy (no BPTT kernels)"
    with pytest.raises(TypeError):
        GaussianGRUPolicy(_spec(), bptt_kernel=True)


def test_scatter_gather_round_trip_through_the_padded_layout():
    from rllab_amd.policies.fused_gru_ops import FusedGRUOps
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    pol = GaussianGRUPolicy(_spec(13, 2), hidden_sizes=(20,), bptt_kernels=True)
    pol.flat_params = pol.flat_params.detach().cpu()
    ops = FusedGRUOps(pol)
    idx, size = pol.pad_index()
    assert ops.n_flat == pol.flat_params.numel() and ops.n_kernel == size
    assert size == 32 + 3 * (15 * 32 + 32 * 32 + 32) + 32 * 2 + 2 + 2
    v = torch.as_tensor(np.random.RandomState(0).randn(ops.n_flat) + 3.0)            # no zero among them
    k = ops.scatter(v)
    assert k.dtype == torch.float32 and k.numel() == size
    assert torch.equal(ops.gather(k), v.float())
    pad = np.ones(size, dtype=bool)
    pad[idx] = False
    assert pad.sum() == size - ops.n_flat > 0
    assert bool(torch.all(k[torch.as_tensor(pad)] == 0)) and bool(torch.all(k[torch.as_tensor(~pad)] != 0))
    # the frozen entries: h0
    assert ops.frozen.tolist() == list(range(20))
    # a width that needs no padding: the vector itself
    full = GaussianGRUPolicy(_spec(), hidden_sizes=(32,), bptt_kernels=True)
    full.flat_params = full.flat_params.detach().cpu()
    o32 = FusedGRUOps(full)
    assert o32.index is None and o32.n_kernel == o32.n_flat
    w = torch.randn(o32.n_flat, dtype=torch.float64)
    assert torch.equal(o32.gather(o32.scatter(w)), w.float())


def test_a_batch_the_kernels_do_not_take_is_named_in_the_log(tmp_path):
    """``accepts`` is asked by the optimizer after init_opt has logged the kernels' line: a refused tuple says so, once."""
    from rllab_amd.misc import logger
    from rllab_amd.policies.fused_gru_ops import FusedGRUOps
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    pol = GaussianGRUPolicy(_spec(), bptt_kernels=True)
    pol.flat_params = pol.flat_params.detach().cpu()
    ops = FusedGRUOps(pol)
    T, N = 3, 5
    inputs = (torch.zeros(4, T, N), torch.zeros(1, T, N), torch.zeros(T, N), torch.zeros(1, T, N), torch.zeros(1, 1, 1),
              torch.ones(T, N, dtype=torch.bool), torch.ones(T, N), torch.tensor(1.0 / (T * N), dtype=torch.float64))
    txt = str(tmp_path / "log.txt")
    logger.add_text_output(txt)
    logger.set_quiet(True)
    try:
        assert not ops.accepts(inputs) and not ops.accepts(inputs)             # planes on the CPU
    finally:
        logger.remove_text_output(txt)
        logger.set_quiet(False)
    assert open(txt).read().count("update path: torch autograd for this batch") == 1
