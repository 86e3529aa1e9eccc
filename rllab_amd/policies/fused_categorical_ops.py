"""HIP-kernel loss / gradient / Fisher-vector product for a CategoricalMLPPolicy
(rllab/policies/categorical_mlp_policy.py:15-85 with rllab/distributions/categorical.py:23-87).

The logit network runs as a plain function on planes (policies/planes_ops.py::PlanesOps over one KernelNet), the categorical
head after it is ``rl_categorical_head`` / ``rl_categorical_fisher`` (csrc/categorical_kernels.hip):

    loss, KL   : forward -> head (sums only)
    gradient   : forward -> head (sums + cotangent on the logit planes) -> backward
    F v        : forward-with-tangent -> Fisher head (Hessian of the per-sample KL in the logits at old == new) -> backward

The network: one, two or three tanh layers of at most 128 units, run zero-padded to 32 / 64 / 128 per layer (exact:
policies/kernel_layout.py::mlp_pad_index), flat_dim <= 30 inputs, at most 8 actions.  Inputs: the categorical update batch of
policies/update_batch.py.
"""
import torch

from rllab_amd import _lib
from rllab_amd.policies.planes_ops import PlanesOps
from rllab_amd.policies.update_batch import CategoricalBatch
from rllab_amd.sampler import dist as D


class FusedCategoricalOps(PlanesOps):
    PLANES = (("logits", "dlogits", "glogits"),)
    HEAD_WORKSPACE_BYTES = "rl_categorical_head_workspace_bytes"

    @staticmethod
    def supported(policy):
        return policy.why_no_kernel_layout() is None

    def __init__(self, policy):
        net = policy.kernel_net()
        assert net is not None
        super(FusedCategoricalOps, self).__init__(policy, [net])

    def accepts(self, inputs):
        """One-hot observation and action planes, recorded probabilities, on the device."""
        if len(inputs) != len(CategoricalBatch._fields):
            return False
        b = CategoricalBatch._make(inputs)
        return b.obs.is_cuda and b.old_prob.dim() == 2 and b.old_prob.shape[0] == self.dims[1] and \
            b.obs.shape[0] == self.dims[0] and not D.is_distributed()

    def _tensors(self, inputs):
        b = CategoricalBatch._make(inputs)
        return {k: getattr(b, k).float().contiguous() for k in ("obs", "actions", "advantages", "old_prob", "weights")}

    def _head(self, b, inv, out4, vpg=False, penalty=0.0, with_cotangents=False):
        p, t = b["planes"], b["tensors"]
        _lib.check(_lib.lib.rl_categorical_head(
            b["B"], self.dims[1], _lib.ptr(p["logits"]), _lib.ptr(t["actions"]), _lib.ptr(t["advantages"]),
            _lib.ptr(t["old_prob"]), _lib.ptr(t["weights"]), inv, int(bool(vpg)), float(penalty),
            _lib.ptr(p["glogits"]) if with_cotangents else None, _lib.ptr(self._head_ws), self._head_ws.numel(),
            _lib.ptr(out4), _lib.stream_ptr()), "rl_categorical_head")

    def _fisher_head(self, b):
        p = b["planes"]
        _lib.check(_lib.lib.rl_categorical_fisher(b["B"], self.dims[1], _lib.ptr(p["dlogits"]), _lib.ptr(p["logits"]),
                                                  _lib.ptr(b["tensors"]["weights"]), float(b["structs"][0].inv_count),
                                                  _lib.ptr(p["glogits"]), _lib.stream_ptr()), "rl_categorical_fisher")

    def value_and_grad(self, inputs, penalty=0.0, vpg=False):
        assert not (vpg and penalty), "the log-likelihood objective has no KL penalty"
        g = self.loss_grad(inputs, vpg=vpg, penalty=penalty)
        _, _, inv = self._batch(inputs)
        host = torch.cat([self._last_out4[:3], g]).cpu().numpy()          # one read: the sums and the gradient
        if vpg:
            return float(-host[2] * inv), host[3:].copy()
        return float((-host[0] + penalty * host[1]) * inv), host[3:].copy()
