"""HIP-kernel loss / gradient / Fisher-vector product of a CategoricalGRUPolicy for ConjugateGradientOptimizer (TRPO,
TNPG).

The three passes of csrc/categorical_gru_bptt_kernels.hip on the dense [., T, N] planes of a recurrent categorical update
batch (policies/update_batch.py; one-hot observations [S, T, N] and actions [4, T, N]).

    loss, KL   : rl_gru_categorical_eval   one forward sweep (every line-search candidate)
    gradient   : rl_gru_categorical_grad   forward sweep, backward sweep, the weight sums on the matrix cores; also loss, KL
    F v        : rl_gru_categorical_fvp    tangent sweep next to the h planes the gradient pass left, the same backward half

The kernels read the one-hot planes as INDEX planes: ``argmax`` over the one-hot axis, taken once per batch.  Everything
else -- the padded layout, the descriptor and loss caches, the passes -- is ``RecurrentOpsBase`` (policies/fused_gru_ops.py).
"""
import torch

from rllab_amd import _lib
from rllab_amd.misc import logger
from rllab_amd.policies.fused_gru_ops import RecurrentOpsBase
from rllab_amd.policies.update_batch import RecurrentCategoricalBatch as Batch
from rllab_amd.sampler import dist as D


class FusedCategoricalGRUOps(RecurrentOpsBase):
    ENTRY = ("rl_gru_categorical_eval", "rl_gru_categorical_grad", "rl_gru_categorical_fvp")
    HEAD_FIELD = "prob"

    def __init__(self, policy):
        RecurrentOpsBase.__init__(self, policy)
        # (n_states, n_act, hidden, include_action)
        self.dims = (int(policy.obs_dim), int(policy.action_dim), int(policy.kernel_hidden),
                     int(policy.state_include_action))

    def accepts(self, inputs):
        """A recurrent categorical batch of [., T, N] planes on the device.  A tuple that is not one falls back to autograd
        inside the optimizer, behind init_opt's ``update path: HIP kernels`` line: the log says so, once per tuple."""
        b = Batch._make(inputs) if len(inputs) == len(Batch._fields) else None
        ok = b is not None and b.obs.is_cuda and b.obs.dim() == 3 and b.obs.shape[0] == self.dims[0] \
            and b.actions.dim() == 3 and b.actions.shape[0] == self.dims[1] and b.old_prob.shape == b.actions.shape \
            and not D.is_distributed()
        key = id(inputs[0]) if len(inputs) else 0
        if not ok and getattr(self, "_refused_key", None) != key:
            self._refused_key = key
            logger.log("update path: torch autograd for this batch -- its planes are not the [., T, N] device planes "
                       "that FusedCategoricalGRUOps takes")
        return ok

    def _describe(self, inputs):
        """(descriptor, the tensors it points into, workspace bytes) of an input tuple."""
        named = Batch._make(inputs)
        f32, i32 = torch.float32, torch.int32
        keep = [named.obs.argmax(dim=0).to(i32).contiguous(), named.actions.argmax(dim=0).to(i32).contiguous(),
                named.advantages.to(f32).contiguous(), named.old_prob.to(f32).contiguous(),
                named.start.to(torch.uint8).contiguous(), named.weights.to(f32).contiguous()]
        S, A, H, inc = self.dims
        T, N = int(named.obs.shape[1]), int(named.obs.shape[2])
        need = _lib.lib.rl_gru_categorical_workspace_bytes(N, T, S, H, inc)
        if need == 0:
            raise RuntimeError("rl_gru_categorical_workspace_bytes: %s" % _lib.lib.rl_last_error().decode())
        b = _lib.GruCategoricalBatch(n_envs=N, horizon=T, n_states=S, n_act=A, hidden=H, include_action=inc,
                                     inv_count=float(named.inv_count), state=keep[0].data_ptr(), action=keep[1].data_ptr(),
                                     advantages=keep[2].data_ptr(), old_prob=keep[3].data_ptr(), start=keep[4].data_ptr(),
                                     weights=keep[5].data_ptr())
        return b, keep, need

    def forward_probs(self, inputs, with_grad=False):
        """The probabilities [4, T, N] the forward sweep of the loss pass (``with_grad``: of the gradient pass) computes."""
        prob = torch.empty_like(Batch._make(inputs).old_prob, dtype=torch.float32).contiguous()
        if with_grad:
            self.loss_grad(inputs, means=prob)
        else:
            self._loss_eval(inputs, means=prob)
        return prob
