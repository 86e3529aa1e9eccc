"""HIP-kernel loss / gradient / Fisher-vector product of a GaussianGRUPolicy for ConjugateGradientOptimizer (TRPO, TNPG).

The three passes of csrc/gru_bptt_kernels.hip on the dense [., T, N] planes of a recurrent Gaussian update batch
(policies/update_batch.py; one old log_std row [Da]).

    loss, KL   : rl_gru_gaussian_eval   one forward sweep (every line-search candidate)
    gradient   : rl_gru_gaussian_grad   forward sweep, backward sweep, the weight sums on the matrix cores; also loss, KL
    F v        : rl_gru_gaussian_fvp    tangent sweep next to the h planes the gradient pass left, the same backward half

This is the subset of ``FusedGaussianMLPOps``' interface the optimizer calls when it runs ``krylov.cg`` on the host, which
it does here: ``h0`` is frozen, so the optimizer works in the trainable subspace.  The kernels run the policy at
``kernel_hidden`` units; ``scatter`` / ``gather`` move vectors between the flat order and that zero-padded layout
(``GRUPolicyBase.pad_index``).

``RecurrentOpsBase`` is everything here that does not name a distribution; ``FusedGRUOps`` adds the Gaussian descriptor and
``policies/fused_categorical_gru_ops.py`` the categorical one.
"""
import ctypes

import numpy as np
import torch

from rllab_amd import _lib
from rllab_amd.misc import logger
from rllab_amd.policies.update_batch import RecurrentGaussianBatch as Batch
from rllab_amd.sampler import dist as D


class RecurrentOpsBase(object):
    """What the update passes of the two GRU policies share (``FusedGRUOps`` here, ``FusedCategoricalGRUOps`` in
    policies/fused_categorical_gru_ops.py): the padded layout, the descriptor cache, the workspace, the loss record, and
    the three passes as calls of the family's entry points.  A subclass names those (``ENTRY``), the field of its
    descriptor that receives the forward sweep's head (``HEAD_FIELD``), and builds the descriptor of a tuple
    (``_describe``) and ``accepts``."""
    device_line_search = False          # the host reads every line-search candidate, as the reference does
    ENTRY = None                        # (eval, grad, fvp): names of the C entry points
    HEAD_FIELD = None

    def __init__(self, policy):
        self.policy = policy
        dev = policy.flat_params.device
        idx, size = policy.pad_index()
        self.n_flat, self.n_kernel = int(policy.flat_params.numel()), int(size)
        assert idx.size == self.n_flat
        self.index = None if policy.kernel_layout_is_flat else \
            torch.as_tensor(idx, dtype=torch.long, device=dev)
        frozen = [np.arange(p.offset, p.offset + p.size) for p in policy.get_params() if not p.tags.get("trainable", False)]
        self.frozen = torch.as_tensor(np.concatenate(frozen), dtype=torch.long, device=dev) if frozen else None
        self._ws = None
        self._bound = {}
        self._loss_cache = None
        self._state_tag = None          # the evaluation point whose h planes the workspace holds

    # -- flat order <-> the kernels' zero-padded layout ---------------------------------------------------------------
    def scatter(self, flat, dtype=torch.float32):
        """A flat vector -> the kernel layout, zeros at the padded places."""
        flat = flat.to(dtype)
        if self.index is None:
            return flat.contiguous()
        out = torch.zeros(self.n_kernel, dtype=dtype, device=flat.device)
        out.index_copy_(0, self.index.to(flat.device), flat)
        return out

    def gather(self, padded):
        """... and back: the real entries of a kernel-layout vector, in flat order."""
        return padded if self.index is None else padded.index_select(0, self.index.to(padded.device))

    # -- the batch ------------------------------------------------------------------------------------------------------
    def _eval_point(self, inputs):
        """(batch, parameter version)."""
        return (tuple(id(t) for t in inputs), self.policy.param_version())

    def _batch(self, inputs):
        """The C-ABI descriptor of an input tuple, built once per tuple; theta is refreshed on every call."""
        theta = self.policy.rollout_layout()
        key = tuple(id(t) for t in inputs)
        hit = self._bound.get(key)
        if hit is None:
            dev = inputs[0].device
            b, keep, need = self._describe(inputs)
            if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
                self._state_tag = None
            self._bound.clear()              # one batch at a time: the workspace is one batch's
            hit = self._bound[key] = (b, keep + list(inputs))
        b = hit[0]
        b.theta = theta.data_ptr()
        b.workspace, b.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        setattr(b, self.HEAD_FIELD, None)
        self._theta_keep = theta
        return b

    def release(self):
        """Drop the cached descriptor (and the batch tensors it keeps alive)."""
        self._bound.clear()
        self._loss_cache = None
        self._state_tag = None

    # -- loss and KL ----------------------------------------------------------------------------------------------------
    def _record(self, tag, out2):
        c = dict(tag=tag, out=out2, host=None)
        self._loss_cache = c
        return c

    @staticmethod
    def _resolve(c):
        if c["host"] is None:
            h = c["out"].cpu().numpy()
            c["host"] = (float(h[0]), float(h[1]))
        return c["host"]

    def _call(self, which, *args):
        name = self.ENTRY[which]
        _lib.check(getattr(_lib.lib, name)(*(args + (_lib.stream_ptr(),))), name)

    def _loss_eval(self, inputs, means=None):
        """``means``: where the forward sweep leaves its head (the means; the probabilities), or None."""
        tag = self._eval_point(inputs)
        c = self._loss_cache
        if means is None and c is not None and c["tag"] == tag:
            return c
        b = self._batch(inputs)
        setattr(b, self.HEAD_FIELD, None if means is None else means.data_ptr())
        out2 = torch.empty(2, dtype=torch.float64, device=inputs[0].device)
        self._call(0, ctypes.byref(b), _lib.ptr(out2))
        return self._record(tag, out2)

    def loss_and_kl(self, inputs):
        """(surrogate loss, mean KL) at the current parameters, as Python floats."""
        return self._resolve(self._loss_eval(inputs))

    def loss_and_kl_deferred(self, inputs):
        """Launch the pass now, read later: ``f() -> (loss, mean KL)``, valid after the parameters move on."""
        c = self._loss_eval(inputs)
        return lambda: self._resolve(c)

    # -- gradient and Fisher-vector product -----------------------------------------------------------------------------
    def loss_grad_kernel(self, inputs, with_loss=False, means=None):
        """The gradient of the surrogate loss in the kernel layout (float32, ``n_kernel`` entries)."""
        tag = self._eval_point(inputs)
        b = self._batch(inputs)
        setattr(b, self.HEAD_FIELD, None if means is None else means.data_ptr())
        dev = inputs[0].device
        out2 = torch.empty(2, dtype=torch.float64, device=dev)
        g = torch.empty(self.n_kernel, dtype=torch.float32, device=dev)
        self._state_tag = None
        self._call(1, ctypes.byref(b), _lib.ptr(out2), _lib.ptr(g))
        self._state_tag = tag
        if with_loss and not (self._loss_cache is not None and self._loss_cache["tag"] == tag):
            self._record(tag, out2)
        self._last_out2 = out2
        return g

    def _mask_frozen(self, g):
        if self.frozen is not None:
            g[self.frozen] = 0.0
        return g

    def loss_grad(self, inputs, keep_activations=False, with_loss=False, means=None):
        """Flat gradient of the surrogate loss (float64, flat order, zeros at the frozen entries).  The pass always leaves
        the h planes for the Fisher-vector products that follow at the same parameters; ``with_loss``: its loss / KL sums
        serve the loss evaluation that belongs to this point."""
        g = self.loss_grad_kernel(inputs, with_loss=with_loss, means=means)
        return self._mask_frozen(self.gather(g).to(torch.float64))

    def fvp_kernel(self, inputs, v_kernel):
        """F v in the kernel layout (float32): the Hessian of the mean KL at new == old times ``v_kernel``."""
        tag = self._eval_point(inputs)
        if self._state_tag != tag:
            self.loss_grad_kernel(inputs)       # the product reads the h planes of the gradient pass at this point
        b = self._batch(inputs)
        out = torch.empty(self.n_kernel, dtype=torch.float32, device=inputs[0].device)
        v_kernel = v_kernel.contiguous()
        self._call(2, ctypes.byref(b), _lib.ptr(v_kernel), _lib.ptr(out))
        return out

    def fvp(self, inputs, full):
        """F full (float64, flat order), ``full`` a flat vector with zeros at the frozen entries."""
        v = self.scatter(self._mask_frozen(full.detach().clone().to(torch.float64)))
        return self._mask_frozen(self.gather(self.fvp_kernel(inputs, v)).to(torch.float64))

    def hvp_approach(self):
        from rllab_amd.policies.fused_ops import FusedFisherHvp
        return FusedFisherHvp(self)


class FusedGRUOps(RecurrentOpsBase):
    ENTRY = ("rl_gru_gaussian_eval", "rl_gru_gaussian_grad", "rl_gru_gaussian_fvp")
    HEAD_FIELD = "means"

    def __init__(self, policy):
        RecurrentOpsBase.__init__(self, policy)
        self.dims = (int(policy.kernel_obs_dim), int(policy.action_dim), int(policy.kernel_hidden),
                     int(policy.state_include_action))
        # a policy on kept observation rows: the batch's [k, T, N] planes go to their rows of zeroed [Do, T, N] planes
        self.obs_rows = None if policy.sensor_rows is None else \
            torch.as_tensor(policy.sensor_rows[1], dtype=torch.long, device=policy.flat_params.device)
        self.batch_obs_dim = int(policy.obs_dim)

    def accepts(self, inputs):
        """A recurrent Gaussian batch of [., T, N] planes on the device with ONE old log_std row.  A tuple that is not one
        falls back to autograd inside the optimizer, behind init_opt's ``update path: HIP kernels`` line: the log says so,
        once per tuple."""
        b = Batch._make(inputs) if len(inputs) == len(Batch._fields) else None
        ok = b is not None and b.obs.is_cuda and b.obs.dim() == 3 and b.obs.shape[0] == self.batch_obs_dim \
            and b.old_log_std.numel() == self.dims[1] and not D.is_distributed()
        key = id(inputs[0]) if len(inputs) else 0
        if not ok and getattr(self, "_refused_key", None) != key:
            self._refused_key = key
            logger.log("update path: torch autograd for this batch -- its planes are not the [., T, N] device planes "
                       "with one old log_std row that FusedGRUOps takes")
        return ok

    def _describe(self, inputs):
        """(descriptor, the tensors it points into, workspace bytes) of an input tuple."""
        named = Batch._make(inputs)
        f32 = torch.float32
        keep = [named.obs.to(f32).contiguous(), named.actions.to(f32).contiguous(), named.advantages.to(f32).contiguous(),
                named.old_mean.to(f32).contiguous(), named.old_log_std.reshape(-1).to(f32).contiguous(),
                named.start.to(torch.uint8).contiguous(), named.weights.to(f32).contiguous()]
        do, da, H, inc = self.dims
        T, N = int(named.obs.shape[1]), int(named.obs.shape[2])
        if self.obs_rows is not None:
            # the occluded rows are zeros that meet zero weight rows; their gradient / product entries are never gathered
            full = torch.zeros((do, T, N), dtype=f32, device=keep[0].device)
            full.index_copy_(0, self.obs_rows.to(full.device), keep[0])
            keep[0] = full
        need = _lib.lib.rl_gru_workspace_bytes(N, T, do, da, H, inc)
        if need == 0:
            raise RuntimeError("rl_gru_workspace_bytes: %s" % _lib.lib.rl_last_error().decode())
        b = _lib.GruBatch(n_envs=N, horizon=T, obs_dim=do, act_dim=da, hidden=H, include_action=inc,
                          inv_count=float(named.inv_count), obs=keep[0].data_ptr(), actions=keep[1].data_ptr(),
                          advantages=keep[2].data_ptr(), old_means=keep[3].data_ptr(), old_log_std=keep[4].data_ptr(),
                          start=keep[5].data_ptr(), weights=keep[6].data_ptr())
        return b, keep, need

    def forward_means(self, inputs, with_grad=False):
        """The means [Da, T, N] the forward sweep of the loss pass (``with_grad``: of the gradient pass) computes."""
        means = torch.empty_like(Batch._make(inputs).old_mean, dtype=torch.float32).contiguous()
        if with_grad:
            self.loss_grad(inputs, means=means)
        else:
            self._loss_eval(inputs, means=means)
        return means
