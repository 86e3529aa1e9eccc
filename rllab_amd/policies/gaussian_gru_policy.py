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
through torch autograd on ``dist_info_planes``, a scan over the time axis of the dense [T, N] batch planes.
"""
import numpy as np
import torch

from rllab_amd.core.parameterized import Param
from rllab_amd.core.serializable import Serializable
from rllab_amd.distributions.recurrent_diagonal_gaussian import RecurrentDiagonalGaussian
from rllab_amd.misc import logger
from rllab_amd.policies.base import StochasticPolicy
from rllab_amd.policies.gaussian_mlp_policy import _default_device
from rllab_amd.spaces import Box

tanh = torch.tanh
GATES = ("r", "u", "c")
KERNEL_HIDDEN = (32, 64)          # the hidden widths the recurrent rollout is built for (narrower: zero padding)


def gru_param_specs(input_dim, hidden, action_dim, learn_std=True):
    """[(name, shape, trainable, regularizable)] in the reference's flat order (GRULayer's add_param calls,
    network.py:132-145, with hidden_init_trainable=False; the output DenseLayer; the log-std ParamLayer)."""
    specs = [("h0", (hidden,), False, False)]
    for g in GATES:
        specs += [("W_x" + g, (input_dim, hidden), True, True), ("W_h" + g, (hidden, hidden), True, True),
                  ("b_" + g, (hidden,), True, False)]
    specs += [("output.W", (hidden, action_dim), True, True), ("output.b", (action_dim,), True, False),
              ("output_log_std.param", (action_dim,), bool(learn_std), True)]
    return specs


class GaussianGRUPolicy(StochasticPolicy, Serializable):
    # FiniteDifferenceHvp (the reference's recurrent example runs it with base_eps = 1e-5) differences two gradients at
    # theta +- eps x with eps = base_eps / |theta| ~ 1e-6.  In the parameters' float32 the shift of an entry is a few ulps of
    # that entry and the difference of the two gradients is mostly rounding: the same update on the CPU gained 169 in
    # AverageReturn over ten iterations in float32 against 399 in float64.  So the two shifted gradients of THIS policy are
    # evaluated in float64 (dist_info_planes runs in the dtype of the vector it is given); parameters, loss, gradient and
    # line search stay float32.
    fd_hvp_dtype = torch.float64

    def __init__(self, env_spec, hidden_sizes=(32,), state_include_action=True, hidden_nonlinearity=tanh,
                 learn_std=True, init_std=1.0, output_nonlinearity=None):
        Serializable.quick_init(self, locals())
        assert isinstance(env_spec.action_space, Box)
        StochasticPolicy.__init__(self, env_spec)
        assert len(hidden_sizes) == 1
        self.obs_dim = env_spec.observation_space.flat_dim
        self.action_dim = env_spec.action_space.flat_dim
        self._state_include_action = bool(state_include_action)
        self.input_dim = self.obs_dim + (self.action_dim if self._state_include_action else 0)
        self.hidden_dim = int(hidden_sizes[0])
        self._hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.hidden_nonlinearity = hidden_nonlinearity
        self.output_nonlinearity = output_nonlinearity
        self.learn_std = learn_std
        self.min_std = None
        self._dist = RecurrentDiagonalGaussian(self.action_dim)

        self._params, off = [], 0
        for name, shape, trainable, regularizable in gru_param_specs(self.input_dim, self.hidden_dim, self.action_dim,
                                                                    learn_std):
            p = Param(name, shape, off, trainable=trainable, regularizable=regularizable)
            p._owner = self
            off += p.size
            self._params.append(p)
        self._by_name = {p.name: p for p in self._params}
        # host-side init with np.random (so a CPU yardstick and the GPU share theta under a seed)
        flat = np.zeros(off, dtype=np.float32)
        for p in self._params:
            if len(p.shape) == 2:
                bound = np.sqrt(6.0 / (p.shape[0] + p.shape[1]))
                flat[p.offset:p.offset + p.size] = np.random.uniform(-bound, bound, size=p.shape).reshape(-1)
        ls = self._by_name["output_log_std.param"]
        flat[ls.offset:ls.offset + ls.size] = np.log(init_std)
        self.flat_params = torch.tensor(flat, dtype=torch.float32, device=_default_device())
        self.reset()

    # -- Parameterized ----------------------------------------------------------------------------------------------
    def get_params_internal(self, **tags):
        return [p for p in self._params if all(p.tags.get(k, False) == v for k, v in tags.items())]

    @property
    def vectorized(self):
        return True

    @property
    def recurrent(self):
        return True

    @property
    def distribution(self):
        return self._dist

    @property
    def state_info_keys(self):
        return ["prev_action"] if self._state_include_action else []

    @property
    def state_include_action(self):
        return self._state_include_action

    def param_version(self):
        """Changes whenever the parameters do: torch's in-place version counter plus the writes the kernels make through
        raw pointers (rl_adam_step), which torch cannot see."""
        return (self.flat_params._version, getattr(self, "_raw_writes", 0))

    def note_raw_write(self):
        self._raw_writes = getattr(self, "_raw_writes", 0) + 1

    # -- forward ------------------------------------------------------------------------------------------------------
    def _views(self, flat):
        """The named parameters as views of ``flat``, the hidden axis zero-padded to the next multiple of 32 -- the widths
        the rollout kernel runs at.  A padded unit has zero weights and bias: c = tanh(0) = 0, it starts at h0 = 0, so
        h' = (1 - u) 0 + u 0 stays 0 and feeds nothing.  Evaluating the forward pass at the padded width makes a narrow
        policy and its zero-padded kernel layout the SAME arithmetic (same operand shapes and values in every product),
        not merely the same function."""
        v = {p.name: p.view(flat) for p in self._params}
        pad = (-self.hidden_dim) % 32
        if pad:
            zp = torch.nn.functional.pad
            for name in list(v):
                if name == "output.W":
                    v[name] = zp(v[name], (0, 0, 0, pad))
                elif name.startswith("W_h"):
                    v[name] = zp(v[name], (0, pad, 0, pad))
                elif name not in ("output.b", "output_log_std.param"):
                    v[name] = zp(v[name], (0, pad))
        return v

    def _act(self, z):
        return z if self.hidden_nonlinearity is None else self.hidden_nonlinearity(z)

    def step_planes(self, x, h, v):
        """One GRU step on planes: x [DI, N], h [H, N] -> (h' [H, N], mean [Da, N]), ``v`` from ``_views`` (H padded)."""
        r = torch.sigmoid(v["W_xr"].t() @ x + v["W_hr"].t() @ h + v["b_r"][:, None])
        u = torch.sigmoid(v["W_xu"].t() @ x + v["W_hu"].t() @ h + v["b_u"][:, None])
        c = self._act(v["W_xc"].t() @ x + r * (v["W_hc"].t() @ h) + v["b_c"][:, None])
        h = (1 - u) * h + u * c
        mean = v["output.W"].t() @ h + v["output.b"][:, None]
        if self.output_nonlinearity is not None:
            mean = self.output_nonlinearity(mean)
        return h, mean

    def dist_info_planes(self, obs, actions, start, flat=None):
        """obs [Do, T, N], actions [Da, T, N], start [T, N] bool (a path begins at (t, n)) -> dict(mean [Da, T, N],
        log_std [Da, 1, 1]): the scan over t of every env column, with ``h`` put back to ``h0`` and ``prev_action`` to 0
        wherever a path starts (``prev_action[t] = actions[t-1]`` elsewhere; row 0 starts a path in every column).  In the
        dtype of ``flat``, differentiable twice.  This is the DEFINITION the rollout kernel and the update are both
        tested against."""
        flat = self.flat_params if flat is None else flat
        dt = flat.dtype
        v = self._views(flat)
        obs, actions = obs.to(dt), actions.to(dt)
        T, N = obs.shape[1], obs.shape[2]
        start = torch.as_tensor(start, device=obs.device).bool()
        h0 = v["h0"][:, None]
        h = h0.expand(h0.shape[0], N)
        zeros = torch.zeros((self.action_dim, N), dtype=dt, device=obs.device)
        means = []
        for t in range(T):
            if t > 0:
                st = start[t][None, :]
                h = torch.where(st, h0, h)
            x = obs[:, t]
            if self._state_include_action:
                pa = zeros if t == 0 else torch.where(st, zeros, actions[:, t - 1])
                x = torch.cat([x, pa], dim=0)
            h, mean = self.step_planes(x, h, v)
            means.append(mean)
        return dict(mean=torch.stack(means, dim=1), log_std=v["output_log_std.param"][:, None, None])

    def dist_info_sym(self, obs_var, state_info_vars=None):
        """The reference-shaped wrapper: obs [N, T, Do] (one padded path per row) and ``state_info_vars["prev_action"]``
        [N, T, Da] -> dict(mean [N, T, Da], log_std [N, T, Da]) (gaussian_gru_policy.py:98-110)."""
        dt, dev = self.flat_params.dtype, self.flat_params.device
        obs = torch.as_tensor(obs_var, dtype=dt, device=dev)
        n, T = obs.shape[0], obs.shape[1]
        obs = obs.reshape(n, T, -1).permute(2, 1, 0)
        start = torch.zeros((T, n), dtype=torch.bool, device=dev)
        start[0] = True
        if self._state_include_action:
            prev = torch.as_tensor(state_info_vars["prev_action"], dtype=dt, device=dev).reshape(n, T, -1).permute(2, 1, 0)
            # dist_info_planes takes the actions themselves: actions[t - 1] = prev_action[t]
            actions = torch.cat([prev[:, 1:], torch.zeros_like(prev[:, :1])], dim=1)
        else:
            actions = torch.zeros((self.action_dim, T, n), dtype=dt, device=dev)
        d = self.dist_info_planes(obs, actions, start)
        mean = d["mean"].permute(2, 1, 0)
        return dict(mean=mean, log_std=d["log_std"].permute(2, 1, 0).expand_as(mean))

    # -- host stepping (sim_policy, tests; sampling runs in the fused rollout) ------------------------------------
    def _host_values(self):
        tag = self.param_version()
        cached = getattr(self, "_host_cache", None)
        if cached is None or cached[0] != tag:
            flat = self.flat_params.detach().cpu().to(torch.float64)
            cached = (tag, flat, self._views(flat))
            self._host_cache = cached
        return cached[2]

    def reset(self, dones=None):
        """``reset()``: one env, back to h0 and no previous action (gaussian_gru_policy.py:112-114).  ``reset(dones)``:
        the vectorised form -- the rows of ``dones`` go back, the buffers are (re)sized to ``len(dones)``."""
        h0 = self._host_values()["h0"].numpy()
        if dones is None:
            dones = [True]
        dones = np.asarray(dones, dtype=bool)
        if getattr(self, "_prev_hiddens", None) is None or len(dones) != len(self._prev_hiddens):
            self._prev_actions = np.zeros((len(dones), self.action_dim))
            self._prev_hiddens = np.zeros((len(dones), h0.size))
        self._prev_actions[dones] = 0.0
        self._prev_hiddens[dones] = h0

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

    def get_action(self, observation):
        actions, agent_infos = self.get_actions([observation])
        return actions[0], {k: v[0] for k, v in agent_infos.items()}

    def recorded_log_std(self):
        """The log_std row a rollout records as agent_info: always a COPY (the update rewrites ``flat_params`` in place)."""
        return self._by_name["output_log_std.param"].view(self.flat_params).detach().clone()

    def log_diagnostics(self, paths):
        traj = getattr(paths, "traj", None)
        if traj is not None and getattr(traj, "log_std_host", None) is not None:
            logger.record_tabular('AveragePolicyStd', float(np.mean(np.exp(traj.log_std_host))))
            return
        logger.record_tabular('AveragePolicyStd', float(torch.exp(self.recorded_log_std().double()).mean()))

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
        if self.obs_dim > MAX_OBS_DIM or self.action_dim > MAX_ACT_DIM:
            return "obs_dim %d / action_dim %d exceed the kernels' %d / %d" % (self.obs_dim, self.action_dim, MAX_OBS_DIM,
                                                                             MAX_ACT_DIM)
        if not self.flat_params.is_cuda or self.flat_params.dtype != torch.float32:
            return "the parameters are not float32 on a HIP device"
        return None

    def why_no_kernel_layout(self):
        """Why the UPDATE of this policy runs through torch autograd (algos/npo.py::log_update_path)."""
        return "recurrent policy (no BPTT kernels)"

    @property
    def kernel_hidden(self):
        """The hidden width the kernel runs this policy at: the next of 32 / 64."""
        return next((H for H in KERNEL_HIDDEN if self.hidden_dim <= H), None)

    def pad_index(self):
        """Index of every parameter inside the kernel's vector: the same order with the hidden axis zero-padded to
        ``kernel_hidden``.  Exact: a padded unit has zero weights and bias, so c = tanh(0) = 0, it starts at h0 = 0 and
        h' = (1 - u) 0 + u 0 stays 0; its outgoing weights are 0."""
        H, Hp = self.hidden_dim, self.kernel_hidden
        idx, off = [], 0
        for name, shape, _, _ in gru_param_specs(self.input_dim, H, self.action_dim):
            rows = 1 if len(shape) == 1 else shape[0]
            cols = shape[-1]
            if name in ("output.b", "output_log_std.param"):
                rows_p, cols_p = 1, cols
            elif name == "output.W":
                rows_p, cols_p = Hp, cols
            elif name.startswith("W_h"):
                rows_p, cols_p = Hp, Hp
            else:                                   # h0, b_*: one row; W_x*: one row per input
                rows_p, cols_p = rows, Hp
            r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
            idx.append((off + r * cols_p + c).reshape(-1))
            off += rows_p * cols_p
        return np.concatenate(idx), off

    def rollout_layout(self):
        """The kernel's parameter vector (float32, device, refreshed when the parameters have moved), or None when the
        recurrent rollout kernel does not run this policy (``why_no_rollout_kernel()`` says why)."""
        if self.why_no_rollout_kernel() is not None:
            return None
        if self.hidden_dim == self.kernel_hidden:
            return self.flat_params.detach()
        lay = getattr(self, "_rollout_layout", None)
        if lay is None:
            idx, size = self.pad_index()
            dev = self.flat_params.device
            lay = dict(idx=torch.as_tensor(idx, dtype=torch.long, device=dev),
                       buf=torch.zeros(size, dtype=torch.float32, device=dev), tag=None)
            self._rollout_layout = lay
        tag = self.param_version()
        if lay["tag"] != tag:
            lay["buf"].index_copy_(0, lay["idx"], self.flat_params.detach())
            lay["tag"] = tag
        return lay["buf"]
