"""CategoricalGRUPolicy (API of rllab/policies/categorical_gru_policy.py:18-188).

prob = softmax(linear(GRU(x))) over a ``Discrete`` action space.  The reference builds this with Lasagne (``GRUNetwork``
with a softmax output, rllab/core/network.py:104-270); here all parameters live in ONE flat float32 device vector in the
reference's flat order

    h0, W_xr, W_hr, b_r, W_xu, W_hu, b_u, W_xc, W_hc, b_c, W_out, b_out

-- ``GaussianGRUPolicy``'s vector without the log-std row (``gru_param_specs(.., log_std_row=False)``) -- with every W
stored [in, out] row-major, Glorot-uniform weights, zero biases and h0.  One step on x = [onehot(obs), onehot(prev_action)]
(the observation alone with ``state_include_action=False``) is the GRU step of network.py:150-155 followed by
``prob = softmax(h' W_out + b_out)``.  ``prev_action`` is the SAMPLED action of the previous step of the same path and
zeros at a path start; ``h`` is ``h0`` at a path start.  Sampling runs in the fused recurrent GridWorld rollout
(csrc/categorical_gru_kernels.hip, ``rollout_layout``); the update runs through torch autograd on ``dist_info_planes``, a
scan over the time axis of the dense [T, N] batch planes -- or, with the engine option ``bptt_kernels=True`` and a
ConjugateGradientOptimizer (TRPO, TNPG), on the back-propagation-through-time and Fisher-vector kernels of
csrc/categorical_gru_bptt_kernels.hip (policies/fused_categorical_gru_ops.py).
"""
import numpy as np
import torch

from rllab_amd.core.serializable import Serializable
from rllab_amd.distributions.recurrent_categorical import RecurrentCategorical
from rllab_amd.policies.base import StochasticPolicy
from rllab_amd.policies.gaussian_mlp_policy import _default_device
from rllab_amd.policies.gru_base import KERNEL_HIDDEN, GRUPolicyBase, gru_param_specs, tanh
from rllab_amd.spaces import Discrete
from rllab_amd.spaces.discrete import weighted_sample

LDS_BYTES = 160 * 1024            # of a CU: the kernel keeps the weights and two [H][64] hidden tiles there


class CategoricalGRUPolicy(GRUPolicyBase, StochasticPolicy, Serializable):
    def __init__(self, env_spec, hidden_dim=32, feature_network=None, state_include_action=True,
                 hidden_nonlinearity=tanh, **kwargs):
        Serializable.quick_init(self, locals())
        # engine option, keyword only: loss, gradient and Fisher-vector products of a TRPO / TNPG update on HIP kernels
        self.bptt_kernels = bool(kwargs.pop("bptt_kernels", False))
        if kwargs:
            raise TypeError("CategoricalGRUPolicy: unexpected arguments %r" % sorted(kwargs))
        assert isinstance(env_spec.action_space, Discrete)
        if feature_network is not None:
            raise NotImplementedError("CategoricalGRUPolicy(feature_network=...): the GRU reads the one-hot observation "
                                      "(and previous action) directly; a feature network in front of it is not built")
        StochasticPolicy.__init__(self, env_spec)
        self.obs_dim = env_spec.observation_space.flat_dim
        self.action_dim = env_spec.action_space.flat_dim
        self._state_include_action = bool(state_include_action)
        self.input_dim = self.obs_dim + (self.action_dim if self._state_include_action else 0)
        self.hidden_dim = int(hidden_dim)
        self.hidden_nonlinearity = hidden_nonlinearity
        self.feature_network = None
        self._dist = RecurrentCategorical(self.action_dim)

        flat = self._build_params()
        self.flat_params = torch.tensor(flat, dtype=torch.float32, device=_default_device())
        self.reset()

    def _specs(self, hidden):
        return gru_param_specs(self.input_dim, hidden, self.action_dim, log_std_row=False)

    @property
    def distribution(self):
        return self._dist

    # -- forward (the step, the scan and the padded views: policies/gru_base.py) ----------------------------------------
    def step_planes(self, x, h, v):
        """One GRU step on planes: x [DI, N], h [H, N] -> (h' [H, N], prob [A, N]), ``v`` from ``_views`` (H padded)."""
        h, logits = self.gru_planes(x, h, v)
        return h, torch.softmax(logits, dim=0)

    def dist_info_planes(self, obs, actions, start, flat=None):
        """obs [S, T, N] one-hot, actions [A, T, N] one-hot, start [T, N] bool (a path begins at (t, n)) -> dict(prob
        [A, T, N]): the scan over t of every env column, with ``h`` put back to ``h0`` and ``prev_action`` to zeros wherever
        a path starts (``prev_action[t] = actions[t-1]`` elsewhere; row 0 starts a path in every column).  In the dtype of
        ``flat``, differentiable twice.  This is the DEFINITION the rollout kernel and the update are both tested
        against."""
        return dict(prob=self._scan_planes(obs, actions, start, flat)[0])

    def dist_info_sym(self, obs_var, state_info_vars=None):
        """The reference-shaped wrapper: obs [N, T, S] (one padded path per row) and ``state_info_vars["prev_action"]``
        [N, T, A] -> dict(prob [N, T, A]) (categorical_gru_policy.py:114-140)."""
        obs, actions, start = self._sym_planes(obs_var, state_info_vars)
        return dict(prob=self.dist_info_planes(obs, actions, start)["prob"].permute(2, 1, 0))

    # -- host stepping (sim_policy, the CPU yardstick, tests; sampling runs in the fused rollout) --------------------
    def get_actions(self, observations):
        """One float64 step of every env on the host; the actions are drawn with ``weighted_sample``
        (rllab/misc/special.py:10-19, one np.random uniform each)."""
        flat_obs = np.asarray(self.observation_space.flatten_n(observations), dtype=np.float64)
        v = self._host_values()
        prev_actions = self._prev_actions.copy()
        x = np.concatenate([flat_obs, prev_actions], axis=-1) if self._state_include_action else flat_obs
        with torch.no_grad():
            h, prob = self.step_planes(torch.as_tensor(x).t(), torch.as_tensor(self._prev_hiddens).t(), v)
        probs, hidden = prob.t().numpy(), h.t().numpy()
        actions = [weighted_sample(p, range(self.action_dim)) for p in probs]
        self._prev_actions = self.action_space.flatten_n(actions)
        self._prev_hiddens = hidden
        agent_info = dict(prob=probs)
        if self._state_include_action:
            agent_info["prev_action"] = prev_actions
        return actions, agent_info

    # -- the update on the recurrent kernels --------------------------------------------------------------------------
    def why_no_kernel_layout(self):
        """Why the UPDATE of this policy runs through torch autograd (algos/npo.py::log_update_path), or None when
        ``bptt_kernels=True`` and the kernels of csrc/categorical_gru_bptt_kernels.hip take it."""
        if not self.bptt_kernels:
            return GRUPolicyBase.why_no_kernel_layout(self)
        if not 1 <= self.hidden_dim <= KERNEL_HIDDEN[-1]:
            return "hidden_dim=%d: the recurrent update kernels run 1 .. %d hidden units" % (
                self.hidden_dim, KERNEL_HIDDEN[-1])
        if self.hidden_nonlinearity is not tanh:
            return "hidden_nonlinearity is %s (the recurrent update kernels evaluate tanh)" % getattr(
                self.hidden_nonlinearity, "__name__", repr(self.hidden_nonlinearity))
        if self.action_dim != 4:
            return "%d actions (the recurrent categorical update kernels are built for GridWorld's 4)" % self.action_dim
        if not self.flat_params.is_cuda or self.flat_params.dtype != torch.float32:
            return "the parameters are not float32 on a HIP device"
        from rllab_amd import _lib
        if _lib.lib.rl_gru_categorical_workspace_bytes(64, 1, self.obs_dim, self.kernel_hidden,
                                                       int(self._state_include_action)) == 0:
            return _lib.lib.rl_last_error().decode()
        return None

    def fused_ops(self):
        """``FusedCategoricalGRUOps`` for a ConjugateGradientOptimizer, or None (then the update runs through torch
        autograd and ``why_no_kernel_layout()`` says why)."""
        if not self.bptt_kernels or self.why_no_kernel_layout() is not None:
            return None
        from rllab_amd.policies.fused_categorical_gru_ops import FusedCategoricalGRUOps
        return FusedCategoricalGRUOps(self)

    # -- what the recurrent rollout kernel reads ----------------------------------------------------------------------
    def kernel_lds_bytes(self):
        """Bytes of LDS the rollout kernel needs for this policy: the padded weights plus two [H][64] hidden tiles."""
        H = self.kernel_hidden
        floats = sum(int(np.prod(shape)) for _, shape, _, _ in self._specs(H))
        return 4 * (floats + 2 * H * 64)

    def why_no_rollout_kernel(self):
        """One sentence naming what keeps this policy off the fused recurrent rollout, or None."""
        if not 1 <= self.hidden_dim <= KERNEL_HIDDEN[-1]:
            return "hidden_dim=%d: the recurrent rollout kernel runs 1 .. %d hidden units" % (
                self.hidden_dim, KERNEL_HIDDEN[-1])
        if self.hidden_nonlinearity is not tanh:
            return "hidden_nonlinearity is %s (the recurrent rollout kernel evaluates tanh)" % getattr(
                self.hidden_nonlinearity, "__name__", repr(self.hidden_nonlinearity))
        if self.kernel_lds_bytes() > LDS_BYTES:
            return "%d observations at hidden_dim=%d: the weights and the hidden state take %d bytes of LDS (a CU has " \
                   "%d)" % (self.obs_dim, self.hidden_dim, self.kernel_lds_bytes(), LDS_BYTES)
        if not self.flat_params.is_cuda or self.flat_params.dtype != torch.float32:
            return "the parameters are not float32 on a HIP device"
        return None
