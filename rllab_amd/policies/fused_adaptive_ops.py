"""HIP-kernel loss / gradient / Fisher-vector product for a GaussianMLPPolicy whose log-std is a NETWORK
(``adaptive_std=True`` or ``std_network=...``, rllab/policies/gaussian_mlp_policy.py:60-98; the configuration of the
reference's regression test tests/regression_tests/test_issue_3.py).

The flat parameter vector is [mean network | std network].  Both networks run as plain functions on planes
(policies/planes_ops.py::PlanesOps over two KernelNets), the diagonal-Gaussian head between them is ``rl_gaussian_head`` /
``rl_gaussian_fisher`` (csrc/gaussian_head_kernels.hip):

    loss, KL   : forward x 2 -> head (sums only)
    gradient   : forward x 2 -> head (sums + cotangents on the mean / log-std planes) -> backward x 2
    F v        : forward-with-tangent x 2 -> Fisher head (diagonal in (mean, log_std) at old == new) -> backward x 2

Each network: one, two or three tanh layers of at most 128 units, run zero-padded to 32 / 64 / 128 per layer (exact: a padded
unit has zero weights and bias, tanh(0) = 0; policies/kernel_layout.py::mlp_pad_index; two equal layers of 32 / 64 on a
HIP-native (obs, action) pair run one wavefront per tile, every other shape the cooperative kernels of
csrc/policy_wide_kernels.hip), obs_dim <= 30, action_dim <= 8.  Inputs: the Gaussian update batch of
policies/update_batch.py with per-sample old log-std planes.
"""
import math

import torch

from rllab_amd import _lib
from rllab_amd.core.network import tanh
from rllab_amd.policies.planes_ops import KernelNet, PlanesOps
from rllab_amd.policies.update_batch import GaussianBatch
from rllab_amd.sampler import dist as D


def _net_ok(net, obs_dim, act_dim):
    # (not KernelNet.why_not: this also asks for a linear output on the policy's own dimensions, and does not ask the
    # library whether the padded shape has a kernel -- the two refuse different policies)
    from rllab_amd.policies.kernel_layout import layer_padded_sizes
    return (layer_padded_sizes(net.hidden_sizes) is not None and net.hidden_nonlinearity is tanh
            and net.output_nonlinearity is None and net.input_dim == obs_dim and net.output_dim == act_dim)


class FusedAdaptiveStdOps(PlanesOps):
    PLANES = (("mean", "dmean", "gmean"), ("lstd", "dlstd", "glstd"))
    HEAD_WORKSPACE_BYTES = "rl_gaussian_head_workspace_bytes"

    @staticmethod
    def supported(policy):
        if not getattr(policy, "state_dependent_std", False) or not policy.flat_params.is_cuda \
                or policy.flat_params.dtype != torch.float32:
            return False
        from rllab_amd.policies.kernel_layout import MAX_ACT_DIM, MAX_OBS_DIM
        if policy.obs_dim > MAX_OBS_DIM or policy.action_dim > MAX_ACT_DIM:
            return False
        return _net_ok(policy._mean_network, policy.obs_dim, policy.action_dim) and \
            _net_ok(policy._std_network, policy.obs_dim, policy.action_dim)

    def __init__(self, policy):
        super(FusedAdaptiveStdOps, self).__init__(policy, [KernelNet(policy, policy._mean_network),
                                                           KernelNet(policy, policy._std_network)])
        # (the networks' structs carry no floor: the Gaussian head takes the policy's as its own argument)
        self.log_min = math.log(policy.min_std) if policy.min_std is not None else -1e30

    @property
    def nets(self):
        """(offset, size, padded hidden triple) of [mean net, std net] in the flat vector."""
        return [(n.offset, n.size, n.hidden3) for n in self.kernel_nets]

    def accepts(self, inputs):
        """Per-sample old log_std planes [Da, B] (what a state-dependent std records)."""
        if len(inputs) != len(GaussianBatch._fields):
            return False
        b = GaussianBatch._make(inputs)
        return b.obs.is_cuda and b.old_log_std.dim() == 2 and b.old_log_std.shape[-1] == b.obs.shape[-1] \
            and b.obs.shape[-1] > 1

    def _tensors(self, inputs):
        b = GaussianBatch._make(inputs)
        return dict(obs=b.obs.contiguous(), actions=b.actions.contiguous(), advantages=b.advantages.contiguous(),
                    old_mean=b.old_mean.contiguous(), old_log_std=b.old_log_std.float().contiguous(),
                    weights=b.weights.contiguous())

    def _head(self, b, inv, out4, vpg=False, penalty=0.0, with_cotangents=False):
        p, t = b["planes"], b["tensors"]
        _lib.check(_lib.lib.rl_gaussian_head(
            b["B"], self.dims[1], _lib.ptr(p["mean"]), _lib.ptr(p["lstd"]), _lib.ptr(t["actions"]), _lib.ptr(t["advantages"]),
            _lib.ptr(t["old_mean"]), _lib.ptr(t["old_log_std"]), _lib.ptr(t["weights"]), inv, self.log_min, int(vpg),
            float(penalty), _lib.ptr(p["gmean"]) if with_cotangents else None,
            _lib.ptr(p["glstd"]) if with_cotangents else None, _lib.ptr(self._head_ws), self._head_ws.numel(),
            _lib.ptr(out4), _lib.stream_ptr()), "rl_gaussian_head")

    def _fisher_head(self, b):
        p = b["planes"]
        _lib.check(_lib.lib.rl_gaussian_fisher(
            b["B"], self.dims[1], _lib.ptr(p["dmean"]), _lib.ptr(p["dlstd"]), _lib.ptr(p["lstd"]),
            _lib.ptr(b["tensors"]["weights"]), float(b["structs"][0].inv_count), self.log_min, _lib.ptr(p["gmean"]),
            _lib.ptr(p["glstd"]), _lib.stream_ptr()), "rl_gaussian_fisher")

    def value_and_grad(self, inputs, penalty=0.0):
        g = self.loss_grad(inputs, penalty=penalty)
        _, _, inv = self._batch(inputs)
        sums = D.all_reduce_sum_(self._last_out4[:3].clone()).cpu().numpy()
        idx = self.policy._flat_index(trainable=True)
        host = g.cpu().numpy()
        return float((-sums[0] + penalty * sums[1]) * inv), (host if idx is None else host[idx.cpu().numpy()]).copy()
