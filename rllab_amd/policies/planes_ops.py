"""Networks as plain functions on planes: what the update passes of a policy made of one or more tanh MLPs share.

``KernelNet`` is the kernels' copy of one network of a policy's flat parameter vector; ``PlanesOps`` runs loss / gradient /
Fisher-vector product as  forward (every network) -> distribution head -> backward (every network)  over ``rl_mlp_forward_ws``
/ ``rl_mlp_backward`` (csrc/policy_kernels.hip, csrc/policy_wide_kernels.hip: modes OUT / OUT_TAN / BWD, which read the
network fields, ``obs`` and ``weights`` of rl_policy_batch and nothing else).  Evaluation caching, the device CG and the line
search writes are ``FusedGaussianMLPOps``'s.  A subclass names its planes and supplies the heads: FusedAdaptiveStdOps (mean
and log-std network, Gaussian head), FusedCategoricalOps (logit network, categorical head).
"""
import ctypes

import torch

from rllab_amd import _lib
from rllab_amd.core.network import tanh
from rllab_amd.policies.fused_ops import FusedGaussianMLPOps
from rllab_amd.sampler import dist as D


class _IdentityLayout(object):
    """The optimizer-facing parameter space IS the policy's flat vector; the networks' zero padding happens per network,
    where their kernel-layout copies are made (``KernelNet``)."""
    wide = False
    exact = True

    def __init__(self, policy):
        self.policy = policy
        self.P = self.P_pad = policy.flat_params.numel()

    def theta(self):
        return self.policy.flat_params.detach()

    def pack(self, vec):
        return vec

    def unpack(self, vec):
        return vec


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

    def part(self, vec):
        """This network's entries of a vector in the policy's flat order (the vector itself when the network is all of it:
        a view costs the host as much as a launch)."""
        return vec if vec.numel() == self.size else vec[self.offset:self.offset + self.size]

    def current(self):
        """The kernel-layout parameter vector at the policy's CURRENT parameters (a persistent buffer)."""
        tag = self.policy.param_version()
        if tag != self._tag:
            self.scatter(self.theta, self.part(self.policy.flat_params.detach()))
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


class PlanesOps(FusedGaussianMLPOps):
    # the loss evaluation is a chain of launches (no single rl_policy_loss_kl to gate): the host reads every line-search
    # candidate, as the reference does
    device_line_search = False
    PLANES = ()                  # per network: names of its (output, tangent, cotangent) planes [out_dim, B]
    HEAD_WORKSPACE_BYTES = None  # the C entry point that sizes the head's workspace

    def __init__(self, policy, nets):
        """``nets``: the KernelNets that make up the policy's flat vector, in its order."""
        self.kernel_nets = nets = list(nets)
        assert [n.offset for n in nets] == [sum(m.size for m in nets[:i]) for i in range(len(nets))]
        assert sum(n.size for n in nets) == policy.flat_params.numel()
        self._bind(policy, _IdentityLayout(policy), (nets[0].in_dim, nets[0].out_dim) + nets[0].hidden3)
        self._head_ws = None

    def _workspace(self, device):
        if self._ws is None or self._ws.device != device:
            self._ws = torch.empty(max(n.workspace_bytes() for n in self.kernel_nets), dtype=torch.uint8, device=device)
            self._head_ws = torch.empty(getattr(_lib.lib, self.HEAD_WORKSPACE_BYTES)(), dtype=torch.uint8, device=device)
        return self._ws

    def _tensors(self, inputs):
        """dict of the contiguous float32 batch tensors the passes read, by field name: ``obs`` first, ``weights`` among them."""
        raise NotImplementedError

    def _batch(self, inputs):
        key = tuple(id(t) for t in inputs)
        hit = self._bound.get(key)
        if hit is not None:
            for st, net in zip(hit[0]["structs"], self.kernel_nets):
                st.theta = net.current().data_ptr()
            return hit
        t = self._tensors(inputs)
        obs, w, inv = t["obs"], t["weights"], float(inputs[-1])
        B, dev = obs.shape[-1], obs.device
        f32 = dict(dtype=torch.float32, device=dev)
        planes = {name: torch.empty((net.out_dim, B), **f32)
                  for net, names in zip(self.kernel_nets, self.PLANES) for name in names}
        # per-network scratch of the passes, allocated once per bound batch (ten Fisher-vector products per update
        # would otherwise allocate and fill four tensors each): the tangent in the kernels' policy layout
        # [network parameters | out_dim zeros] and the float64 gradient row rl_mlp_backward writes
        scratch = [dict(tangent=torch.zeros(n.p_pad + n.out_dim, **f32),
                        grad=torch.empty(n.p_pad + n.out_dim, dtype=torch.float64, device=dev)) for n in self.kernel_nets]
        b = dict(structs=[n.batch_struct(B, obs, w, inv) for n in self.kernel_nets], planes=planes, B=B, scratch=scratch,
                 tensors=t)
        if len(self._bound) >= 2:
            self._bound.clear()
        self._bound[key] = (b, list(t.values()) + list(inputs), inv)
        return self._bound[key]

    # -- the three passes ---------------------------------------------------------------------------------------------
    def _forward(self, b, tangents=None):
        """Every network's output plane (and its tangent in direction ``tangents`` = kernel-layout float32 vectors)."""
        p, ws, st = b["planes"], self._ws, _lib.stream_ptr()         # (the cooperative kernels keep their operand images in ws)
        for i, (name, dname, _) in enumerate(self.PLANES):
            vec = None if tangents is None else _lib.ptr(tangents[i])
            dout = None if tangents is None else _lib.ptr(p[dname])
            _lib.check(_lib.lib.rl_mlp_forward_ws(ctypes.byref(b["structs"][i]), vec, _lib.ptr(ws), ws.numel(),
                                                  _lib.ptr(p[name]), dout, st), "rl_mlp_forward_ws")

    def _head(self, b, inv, out4, vpg=False, penalty=0.0, with_cotangents=False):
        """The four loss sums of the output planes into ``out4`` (and the cotangent planes of the objective)."""
        raise NotImplementedError

    def _fisher_head(self, b):
        """Cotangent planes <- the Fisher metric of the distribution (at old == new) applied to the tangent planes."""
        raise NotImplementedError

    def _backward(self, b, ws, out):
        """out [P] float64 <- every network's gradient of its cotangent plane, side by side."""
        p, st = b["planes"], _lib.stream_ptr()
        for net, struct, sc, (_, _, gname) in zip(self.kernel_nets, b["structs"], b["scratch"], self.PLANES):
            _lib.check(_lib.lib.rl_mlp_backward(ctypes.byref(struct), _lib.ptr(p[gname]), _lib.ptr(ws), ws.numel(),
                                                _lib.ptr(sc["grad"]), st), "rl_mlp_backward")
            net.part(out).copy_(net.gather(sc["grad"]))
        return D.update_sum_(out)                     # (the argument itself in one process)

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
        self._head(b, inv, out4, vpg=vpg, penalty=penalty, with_cotangents=True)
        if with_loss and not (self._loss_cache is not None and self._loss_cache["tag"] == tag):
            self._loss_record(tag, out4, inv)
        self._last_out4 = out4
        return self._backward(b, ws, out)

    def _fvp_into(self, b, ws, vec32, out, inputs=None):
        """F vec: the tangents of every network, the Fisher metric of the head, back through every network."""
        tangents = [sc["tangent"] for sc in b["scratch"]]
        for net, tangent in zip(self.kernel_nets, tangents):   # (padded positions and the trailing out_dim floats stay zero)
            net.scatter(tangent, net.part(vec32))
        self._forward(b, tangents)
        self._fisher_head(b)
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
