"""GaussianGRUPolicy (API of rllab/policies/gaussian_gru_policy.py:17-159).

mean = linear(GRU(x)), log_std = one free row.  The reference builds this with Lasagne (``GRUNetwork`` / ``GRULayer``,
rllab/core/network.py:104-270); here all parameters live in ONE flat float32 device vector in the reference's flat order

    h0, W_xr, W_hr, b_r, W_xu, W_hu, b_u, W_xc, W_hc, b_c, W_out, b_out, log_std

with every W stored [in, out] row-major, Glorot-uniform weights, zero biases and h0, log_std = log(init_std).  One step on
x = [obs, prev_action] (obs alone with ``state_include_action=False``), network.py:150-155:

    r = sigmoid(x W_xr + h W_hr + b_r)          u = sigmoid(x W_xu + h W_hu + b_u)
    c = tanh   (x W_xc + r * (h W_hc) + b_c)    h' = (1 - u) * h + u * c          mean = h' W_out + b_out

``prev_action`` is the SAMPLED action of the previous step of the same path and zeros at a path start; ``h`` is ``h0`` at a
path start.  Sampling runs in the fused recurrent rollout (csrc/gru_kernels.hip, ``rollout_layout``); the update runs
through torch autograd on ``dist_info_planes``, a scan over the time axis of the dense [T, N] batch planes -- or, with the
engine option ``bptt_kernels=True`` and a ConjugateGradientOptimizer (TRPO, TNPG), on the back-propagation-through-time
and Fisher-vector kernels of csrc/gru_bptt_kernels.hip (policies/fused_gru_ops.py).
"""
import numpy as np
import torch

from rllab_amd.core.serializable import Serializable
from rllab_amd.distributions.recurrent_diagonal_gaussian import RecurrentDiagonalGaussian
from rllab_amd.misc import logger
from rllab_amd.policies.base import StochasticPolicy
from rllab_amd.policies.gaussian_mlp_policy import _default_device
from rllab_amd.policies.gru_base import GATES, KERNEL_HIDDEN, GRUPolicyBase, gru_param_specs, tanh  # noqa: F401
from rllab_amd.spaces import Box


class GaussianGRUPolicy(GRUPolicyBase, StochasticPolicy, Serializable):
    def __init__(self, env_spec, hidden_sizes=(32,), state_include_action=True, hidden_nonlinearity=tanh,
                 learn_std=True, init_std=1.0, output_nonlinearity=None, **kwargs):
        Serializable.quick_init(self, locals())
        # engine option, keyword only: loss, gradient and Fisher-vector products of a TRPO / TNPG update on HIP kernels
        self.bptt_kernels = bool(kwargs.pop("bptt_kernels", False))
        if kwargs:
            raise TypeError("GaussianGRUPolicy: unexpected arguments %r" % sorted(kwargs))
        assert isinstance(env_spec.action_space, Box)
        StochasticPolicy.__init__(self, env_spec)
        assert len(hidden_sizes) == 1
        self.obs_dim = env_spec.observation_space.flat_dim
        self.action_dim = env_spec.action_space.flat_dim
        # built on kept rows of a HIP-native env's observation (OcclusionEnv, position_only): the kernels run the policy
        # on the full observation, zero weight rows at the occluded entries (GRUPolicyBase.pad_index)
        self._sensor_rows = getattr(env_spec, "sensor_rows", None)
        if self._sensor_rows is not None:
            full, ids = self._sensor_rows
            if len(ids) != self.obs_dim or len(set(ids)) != len(ids) or not all(0 <= i < full for i in ids):
                raise ValueError("env_spec.sensor_rows = %r does not name %d distinct rows of a %d-entry observation" % (
                    self._sensor_rows, self.obs_dim, full))
        self._state_include_action = bool(state_include_action)
        self.input_dim = self.obs_dim + (self.action_dim if self._state_include_action else 0)
        self.hidden_dim = int(hidden_sizes[0])
        self._hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.hidden_nonlinearity = hidden_nonlinearity
        self.output_nonlinearity = output_nonlinearity
        self.learn_std = learn_std
        self.min_std = None
        self._dist = RecurrentDiagonalGaussian(self.action_dim)

        flat = self._build_params()
        ls = self._by_name["output_log_std.param"]
        flat[ls.offset:ls.offset + ls.size] = np.log(init_std)
        self.flat_params = torch.tensor(flat, dtype=torch.float32, device=_default_device())
        self.reset()

    def _specs(self, hidden):
        return gru_param_specs(self.input_dim, hidden, self.action_dim, self.learn_std)

    @property
    def distribution(self):
        return self._dist

    # -- forward (the step, the scan and the padded views: policies/gru_base.py) ----------------------------------------
    def step_planes(self, x, h, v):
        """One GRU step on planes: x [DI, N], h [H, N] -> (h' [H, N], mean [Da, N]), ``v`` from ``_views`` (H padded)."""
        h, mean = self.gru_planes(x, h, v)
        if self.output_nonlinearity is not None:
            mean = self.output_nonlinearity(mean)
        return h, mean

    def dist_info_planes(self, obs, actions, start, flat=None):
        """obs [Do, T, N], actions [Da, T, N], start [T, N] bool (a path begins at (t, n)) -> dict(mean [Da, T, N],
        log_std [Da, 1, 1]): the scan over t of every env column, with ``h`` put back to ``h0`` and ``prev_action`` to 0
        wherever a path starts (``prev_action[t] = actions[t-1]`` elsewhere; row 0 starts a path in every column).  In the
        dtype of ``flat``, differentiable twice.  This is the DEFINITION the rollout kernel and the update are both
        tested against."""
        means, v = self._scan_planes(obs, actions, start, flat)
        return dict(mean=means, log_std=v["output_log_std.param"][:, None, None])

    def dist_info_sym(self, obs_var, state_info_vars=None):
        """The reference-shaped wrapper: obs [N, T, Do] (one padded path per row) and ``state_info_vars["prev_action"]``
        [N, T, Da] -> dict(mean [N, T, Da], log_std [N, T, Da]) (gaussian_gru_policy.py:98-110)."""
        obs, actions, start = self._sym_planes(obs_var, state_info_vars)
        d = self.dist_info_planes(obs, actions, start)
        mean = d["mean"].permute(2, 1, 0)
        return dict(mean=mean, log_std=d["log_std"].permute(2, 1, 0).expand_as(mean))

    # -- host stepping (sim_policy, tests; sampling runs in the fused rollout) ------------------------------------
    def get_actions(self, observations):
        flat_obs = np.asarray(self.observation_space.flatten_n(observations), dtype=np.float64)
        v = self._host_values()
        prev_actions = self._prev_actions.copy()
        x = np.concatenate([flat_obs, prev_actions], axis=-1) if self._state_include_action else flat_obs
        with torch.no_grad():
            h, mean = self.step_planes(torch.as_tensor(x).t(), torch.as_tensor(self._prev_hiddens).t(), v)
        means, hidden = mean.t().numpy(), h.t().numpy()
        log_stds = np.tile(v["output_log_std.param"].numpy()[None, :], (len(means), 1))
        rnd = np.random.normal(size=means.shape)
        actions = rnd * np.exp(log_stds) + means
        self._prev_actions = self.action_space.flatten_n(actions)
        self._prev_hiddens = hidden
        agent_info = dict(mean=means, log_std=log_stds)
        if self._state_include_action:
            agent_info["prev_action"] = prev_actions
        return actions, agent_info

    def recorded_log_std(self):
        """The log_std row a rollout records as agent_info: always a COPY (the update rewrites ``flat_params`` in place)."""
        return self._by_name["output_log_std.param"].view(self.flat_params).detach().clone()

    def log_diagnostics(self, paths):
        traj = getattr(paths, "traj", None)
        if traj is not None and getattr(traj, "log_std_host", None) is not None:
            logger.record_tabular('AveragePolicyStd', float(np.mean(np.exp(traj.log_std_host))))
            return
        if traj is not None and getattr(traj, "log_std_planes", None) is not None:
            # a population's first paths: every env its own candidate's row (HipVecEnv.rollout_population_recurrent)
            w = traj.valid.to(torch.float64) if getattr(traj, "valid", None) is not None else None
            e = torch.exp(traj.log_std_planes.double())
            val = float(e.mean()) if w is None else float((e * w).sum() / (w.sum() * e.shape[0]).clamp_min(1.0))
            logger.record_tabular('AveragePolicyStd', val)
            return
        logger.record_tabular('AveragePolicyStd', float(torch.exp(self.recorded_log_std().double()).mean()))

    # -- the update on the recurrent kernels --------------------------------------------------------------------------
    def why_no_kernel_layout(self):
        """Why the UPDATE of this policy runs through torch autograd (algos/npo.py::log_update_path), or None when
        ``bptt_kernels=True`` and the kernels of csrc/gru_bptt_kernels.hip take it."""
        if not self.bptt_kernels:
            return GRUPolicyBase.why_no_kernel_layout(self)
        if not 1 <= self.hidden_dim <= KERNEL_HIDDEN[-1]:
            return "hidden_sizes=%r: the recurrent update kernels run 1 .. %d hidden units" % (
                self._hidden_sizes, KERNEL_HIDDEN[-1])
        if self.hidden_nonlinearity is not tanh:
            return "hidden_nonlinearity is %s (the recurrent update kernels evaluate tanh)" % getattr(
                self.hidden_nonlinearity, "__name__", repr(self.hidden_nonlinearity))
        if self.output_nonlinearity is not None:
            return "output_nonlinearity is not None (the output layer of the recurrent update kernels is linear)"
        if not self.flat_params.is_cuda or self.flat_params.dtype != torch.float32:
            return "the parameters are not float32 on a HIP device"
        from rllab_amd import _lib
        if _lib.lib.rl_gru_workspace_bytes(64, 1, self.kernel_obs_dim, self.action_dim, self.kernel_hidden,
                                           int(self._state_include_action)) == 0:
            return _lib.lib.rl_last_error().decode()
        return None

    def fused_ops(self):
        """``FusedGRUOps`` for a ConjugateGradientOptimizer, or None (then the update runs through torch autograd and
        ``why_no_kernel_layout()`` says why)."""
        if not self.bptt_kernels or self.why_no_kernel_layout() is not None:
            return None
        from rllab_amd.policies.fused_gru_ops import FusedGRUOps
        return FusedGRUOps(self)

    # -- what the recurrent rollout kernel reads ----------------------------------------------------------------------
    def why_no_rollout_kernel(self):
        """One sentence naming what keeps this policy off the fused recurrent rollout, or None."""
        from rllab_amd.policies.kernel_layout import MAX_ACT_DIM, MAX_OBS_DIM
        if not 1 <= self.hidden_dim <= KERNEL_HIDDEN[-1]:
            return "hidden_sizes=%r: the recurrent rollout kernel runs 1 .. %d hidden units" % (
                self._hidden_sizes, KERNEL_HIDDEN[-1])
        if self.hidden_nonlinearity is not tanh:
            return "hidden_nonlinearity is %s (the recurrent rollout kernel evaluates tanh)" % getattr(
                self.hidden_nonlinearity, "__name__", repr(self.hidden_nonlinearity))
        if self.output_nonlinearity is not None:
            return "output_nonlinearity is not None (the recurrent rollout kernel's output layer is linear)"
        if self.kernel_obs_dim > MAX_OBS_DIM or self.action_dim > MAX_ACT_DIM:
            return "obs_dim %d / action_dim %d exceed the kernels' %d / %d" % (self.kernel_obs_dim, self.action_dim,
                                                                             MAX_OBS_DIM, MAX_ACT_DIM)
        if not self.flat_params.is_cuda or self.flat_params.dtype != torch.float32:
            return "the parameters are not float32 on a HIP device"
        return None
