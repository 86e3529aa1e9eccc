"""HIP-kernel loss / gradient / Fisher-vector product for a CategoricalMLPPolicy
(rllab/policies/categorical_mlp_policy.py:15-85 with rllab/distributions/categorical.py:23-87).

The logit network runs on the matrix-core kernels as a plain function on planes (``rl_mlp_forward_ws`` /
``rl_mlp_backward``, csrc/policy_kernels.hip), the categorical head after it is ``rl_categorical_head`` /
``rl_categorical_fisher`` (csrc/categorical_kernels.hip):

    loss, KL   : forward -> head (sums only)
    gradient   : forward -> head (sums + cotangent on the logit planes) -> backward
    F v        : forward-with-tangent -> Fisher head (Hessian of the per-sample KL in the logits at old == new) -> backward

Everything else -- evaluation caching, the device CG, the line search writes -- is inherited from
``FusedGaussianMLPOps``; this class replaces its passes the way ``FusedAdaptiveStdOps`` does for two networks.  The
network: one, two or three tanh layers of at most 128 units, run zero-padded to 32 / 64 / 128 per layer (exact:
policies/kernel_layout.py::mlp_pad_index), flat_dim <= 30 inputs, at most 8 actions.  Inputs are the tuples built by
``rllab_amd.algos.npo.npo_inputs`` for a categorical batch: (obs, actions, advantages, old_prob, weights, 1/W).
"""
import ctypes

import torch

from rllab_amd import _lib
from rllab_amd.core.network import tanh
from rllab_amd.policies.fused_adaptive_ops import _IdentityLayout
from rllab_amd.policies.fused_ops import FusedGaussianMLPOps
from rllab_amd.sampler import dist as D


class KernelNet(object):
    """The kernels' copy of one tanh MLP that lives in a policy's flat parameter vector: zero-padded hidden layers
    (a one-hidden-layer net gets the identity as its second layer), in the kernels' policy layout
    [network parameters | act_dim unused floats]; refreshed when the parameters have moved."""

    def __init__(self, policy, net):
        from rllab_amd.policies.kernel_layout import layer_padded_sizes, mlp_identity_ones, mlp_layer_activations, mlp_pad_index
        self.policy, self.net = policy, net
        self.in_dim, self.out_dim = int(net.input_dim), int(net.output_dim)
        hs = tuple(int(h) for h in net.hidden_sizes)
        Hs = layer_padded_sizes(hs)
        assert Hs is not None
        dev = policy.flat_params.device
        self.offset = net.params[0].offset
        self.size = net.end_offset - self.offset
        self.hidden3 = Hs + (0,) * (3 - len(Hs))
        self.layer_activations = mlp_layer_activations(hs)
        idx, p_pad = mlp_pad_index(self.in_dim, hs, Hs, self.out_dim)
        assert idx.size == self.size
        self.p_pad = int(p_pad)
        self.index = None if hs == Hs else torch.as_tensor(idx, dtype=torch.long, device=dev)
        self.theta = torch.zeros(self.p_pad + self.out_dim, dtype=torch.float32, device=dev)
        ones = mlp_identity_ones(self.in_dim, hs, Hs)
        if ones.size:
            self.theta[torch.as_tensor(ones, dtype=torch.long, device=dev)] = 1.0      # W1 = I: constants for good
        self._tag = None

    @staticmethod
    def why_not(policy, net):
        """One sentence naming what keeps ``net`` off the networks-on-planes kernels, or None."""
        from rllab_amd.policies.kernel_layout import MAX_ACT_DIM, MAX_OBS_DIM, layer_padded_sizes
        hs = tuple(int(h) for h in net.hidden_sizes)
        if net.input_dim > MAX_OBS_DIM or net.output_dim > MAX_ACT_DIM:
            return "flat_dim %d / %d actions exceed the kernels' %d / %d" % (net.input_dim, net.output_dim, MAX_OBS_DIM,
                                                                          MAX_ACT_DIM)
        if net.hidden_nonlinearity is not tanh:
            return "hidden_nonlinearity is %s (the networks-on-planes kernels evaluate tanh layers)" % getattr(
                net.hidden_nonlinearity, "__name__", repr(net.hidden_nonlinearity))
        Hs = layer_padded_sizes(hs)
        if Hs is None:
            return "hidden_sizes=%r: the kernels run one, two or three hidden layers of at most 128 units" % (hs,)
        if not policy.flat_params.is_cuda or policy.flat_params.dtype != torch.float32:
            return "the parameters are not float32 on a HIP device"
        H3 = Hs + (0,) * (3 - len(Hs))
        if _lib.lib.rl_policy_workspace_bytes(int(net.input_dim), int(net.output_dim), H3[0], H3[1], H3[2]) == 0:
            return "hidden_sizes=%r (padded to %r) is not a shape the kernels are built for" % (hs, Hs)
        return None

    def current(self):
        """The kernel-layout parameter vector at the policy's CURRENT parameters (a persistent buffer)."""
        tag = self.policy.param_version()
        if tag != self._tag:
            self.scatter(self.theta, self.policy.flat_params.detach()[self.offset:self.offset + self.size])
            self._tag = tag
        return self.theta

    def scatter(self, dst, src):
        """Real parameters -> their places in a (padded) kernel-layout vector ``dst``."""
        if self.index is None:
            dst[:src.numel()].copy_(src)
        else:
            dst.index_copy_(0, self.index, src.to(dst.dtype))

    def gather(self, src):
        """... and back: the real entries of a kernel-layout vector."""
        return src[:self.size] if self.index is None else src.index_select(0, self.index)

    def workspace_bytes(self):
        h = self.hidden3
        return _lib.lib.rl_policy_workspace_bytes(self.in_dim, self.out_dim, h[0], h[1], h[2])

    def batch_struct(self, n_samples, obs, weights, inv_count=1.0):
        h = self.hidden3
        return _lib.PolicyBatch(n_samples=int(n_samples), obs_dim=self.in_dim, act_dim=self.out_dim, hidden0=h[0],
                                hidden1=h[1], hidden2=h[2], inv_count=float(inv_count),
                                layer_activations=self.layer_activations, log_min_std=-1e30, theta=self.current().data_ptr(),
                                obs=obs.data_ptr(), weights=weights.data_ptr())

    def softmax_of_identity(self):
        """prob[out_dim][in_dim] float32: softmax of the network on the identity observation planes -- the policy as a
        table over one-hot observations (rl_mlp_forward_ws, rl_categorical_softmax)."""
        S, A = self.in_dim, self.out_dim
        dev = self.theta.device
        eye = torch.eye(S, dtype=torch.float32, device=dev)
        ones = torch.ones(S, dtype=torch.float32, device=dev)
        ws = torch.empty(self.workspace_bytes(), dtype=torch.uint8, device=dev)
        logits = torch.empty((A, S), dtype=torch.float32, device=dev)
        prob = torch.empty((A, S), dtype=torch.float32, device=dev)
        b = self.batch_struct(S, eye, ones)
        st = _lib.stream_ptr()
        _lib.check(_lib.lib.rl_mlp_forward_ws(ctypes.byref(b), None, _lib.ptr(ws), ws.numel(), _lib.ptr(logits), None, st),
                   "rl_mlp_forward_ws")
        _lib.check(_lib.lib.rl_categorical_softmax(S, A, _lib.ptr(logits), _lib.ptr(prob), st), "rl_categorical_softmax")
        return prob


class FusedCategoricalOps(FusedGaussianMLPOps):
    # the loss evaluation is a chain of launches (no single rl_policy_loss_kl to gate): the host reads every line-search
    # candidate, as the reference does
    device_line_search = False

    @staticmethod
    def supported(policy):
        return policy.why_no_kernel_layout() is None

    def __init__(self, policy):
        self.policy = policy
        self.layout = _IdentityLayout(policy)
        self.net = policy.kernel_net()
        assert self.net is not None and self.net.offset == 0 and self.net.size == policy.flat_params.numel()
        self.dims = (self.net.in_dim, self.net.out_dim) + self.net.hidden3
        self.n_kernel = self.layout.P_pad
        self.wide_kernels = False                        # (the base __init__ is not run: every attribute it sets is set here)
        self._ws = None
        self._head_ws = None
        self._loss_cache = None
        self._bound = {}
        self._acts = None
        self._acts_tag = None

    def accepts(self, inputs):
        """(obs, one-hot actions, advantages, old_prob, weights, 1/W) planes on the device."""
        return len(inputs) == 6 and inputs[0].is_cuda and inputs[3].dim() == 2 and \
            inputs[3].shape[0] == self.dims[1] and inputs[0].shape[0] == self.dims[0] and not D.is_distributed()

    def _workspace(self, device):
        if self._ws is None or self._ws.device != device:
            self._ws = torch.empty(self.net.workspace_bytes(), dtype=torch.uint8, device=device)
            self._head_ws = torch.empty(_lib.lib.rl_categorical_head_workspace_bytes(), dtype=torch.uint8, device=device)
        return self._ws

    def _batch(self, inputs):
        key = tuple(id(t) for t in inputs)
        hit = self._bound.get(key)
        if hit is not None:
            hit[0]["struct"].theta = self.net.current().data_ptr()
            return hit
        obs, act, adv, old_prob, w, inv_count = inputs
        keep = [t.contiguous() for t in (obs.float(), act.float(), adv.float(), old_prob.float(), w.float())]
        obs, act, adv, old_prob, w = keep
        B, da = obs.shape[-1], self.dims[1]
        f32 = dict(dtype=torch.float32, device=obs.device)
        inv = float(inv_count)
        planes = dict(logits=torch.empty((da, B), **f32), dlogits=torch.empty((da, B), **f32),
                      glogits=torch.empty((da, B), **f32))
        b = dict(struct=self.net.batch_struct(B, obs, w, inv), planes=planes, B=B,
                 tangent=torch.zeros(self.net.p_pad + da, **f32),
                 grad=torch.empty(self.net.p_pad + da, dtype=torch.float64, device=obs.device),
                 tensors=dict(obs=obs, act=act, adv=adv, old_prob=old_prob, w=w))
        if len(self._bound) >= 2:
            self._bound.clear()
        self._bound[key] = (b, keep + list(inputs), inv)
        return self._bound[key]

    # -- the three passes ---------------------------------------------------------------------------------------------
    def _forward(self, b, tangent=None):
        p, ws = b["planes"], self._ws
        _lib.check(_lib.lib.rl_mlp_forward_ws(ctypes.byref(b["struct"]), _lib.ptr(tangent), _lib.ptr(ws), ws.numel(),
                                              _lib.ptr(p["logits"]), None if tangent is None else _lib.ptr(p["dlogits"]),
                                              _lib.stream_ptr()), "rl_mlp_forward_ws")

    def _head(self, b, inv, out4, vpg=False, penalty=0.0, with_cotangent=False):
        p, t = b["planes"], b["tensors"]
        _lib.check(_lib.lib.rl_categorical_head(
            b["B"], self.dims[1], _lib.ptr(p["logits"]), _lib.ptr(t["act"]), _lib.ptr(t["adv"]), _lib.ptr(t["old_prob"]),
            _lib.ptr(t["w"]), inv, int(bool(vpg)), float(penalty), _lib.ptr(p["glogits"]) if with_cotangent else None,
            _lib.ptr(self._head_ws), self._head_ws.numel(), _lib.ptr(out4), _lib.stream_ptr()), "rl_categorical_head")

    def _backward(self, b, ws, out):
        """out [P] float64 <- d network of the cotangent planes."""
        _lib.check(_lib.lib.rl_mlp_backward(ctypes.byref(b["struct"]), _lib.ptr(b["planes"]["glogits"]), _lib.ptr(ws),
                                            ws.numel(), _lib.ptr(b["grad"]), _lib.stream_ptr()), "rl_mlp_backward")
        out.copy_(self.net.gather(b["grad"]))
        return out

    def _loss_eval(self, inputs):
        tag = self._eval_point(inputs)
        c = self._loss_cache
        if c is not None and c["tag"] == tag:
            return c
        b, keep, inv = self._batch(inputs)
        self._workspace(keep[0].device)
        out = torch.empty(4, dtype=torch.float64, device=keep[0].device)
        self._forward(b)
        self._head(b, inv, out)
        return self._loss_record(tag, out, inv)

    def loss_grad(self, inputs, vpg=False, keep_activations=False, with_loss=False, penalty=0.0):
        b, keep, inv = self._batch(inputs)
        ws = self._workspace(keep[0].device)
        out = torch.empty(self.n_kernel, dtype=torch.float64, device=keep[0].device)
        out4 = torch.empty(4, dtype=torch.float64, device=keep[0].device)
        tag = self._eval_point(inputs)
        self._forward(b)
        self._head(b, inv, out4, vpg=vpg, penalty=penalty, with_cotangent=True)
        if with_loss and not (self._loss_cache is not None and self._loss_cache["tag"] == tag):
            self._loss_record(tag, out4, inv)
        self._last_out4 = out4
        return self._backward(b, ws, out)

    def value_and_grad(self, inputs, penalty=0.0, vpg=False):
        assert not (vpg and penalty), "the log-likelihood objective has no KL penalty"
        g = self.loss_grad(inputs, vpg=vpg, penalty=penalty)
        _, _, inv = self._batch(inputs)
        host = torch.cat([self._last_out4[:3], g]).cpu().numpy()          # one read: the sums and the gradient
        if vpg:
            return float(-host[2] * inv), host[3:].copy()
        return float((-host[0] + penalty * host[1]) * inv), host[3:].copy()

    def _fvp_into(self, b, ws, vec32, out, inputs=None):
        """F vec: the tangent of the logits, the Hessian of the per-sample KL in the logits, back through the network."""
        self.net.scatter(b["tangent"], vec32)            # (padded positions and the trailing act_dim floats stay zero)
        self._forward(b, b["tangent"])
        p = b["planes"]
        _lib.check(_lib.lib.rl_categorical_fisher(b["B"], self.dims[1], _lib.ptr(p["dlogits"]), _lib.ptr(p["logits"]),
                                                  _lib.ptr(b["tensors"]["w"]), float(b["struct"].inv_count),
                                                  _lib.ptr(p["glogits"]), _lib.stream_ptr()), "rl_categorical_fisher")
        return self._backward(b, ws, out)

    def fvp_variant(self, inputs):
        """The networks-on-planes products run on the f32 matrix instructions (variant 0)."""
        return 0

    def _cg_loop(self, b, ws, inputs, cg_iters, reg_coeff, residual_tol, x, r, p, p32, z, scal, st):
        for _ in range(cg_iters):
            self._fvp_into(b, ws, p32, z, inputs)
            _lib.check(_lib.lib.rl_cg_step(self.n_kernel, _lib.ptr(z), float(reg_coeff), float(residual_tol),
                                           _lib.ptr(x), _lib.ptr(r), _lib.ptr(p), _lib.ptr(p32), _lib.ptr(scal), st),
                       "rl_cg_step")
