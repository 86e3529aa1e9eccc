"""What the two GRU policies share (``GaussianGRUPolicy``, ``CategoricalGRUPolicy``): the flat parameter vector in the
reference's order, the GRU step on planes (rllab/core/network.py:150-155), the scan over the time axis of the dense batch
planes, host stepping state, and the zero-padded layout the recurrent rollout kernels read.

    h0, W_xr, W_hr, b_r, W_xu, W_hu, b_u, W_xc, W_hc, b_c, W_out, b_out [, log_std]

with every W stored [in, out] row-major, Glorot-uniform weights, zero biases and h0.  One step on x:

    r = sigmoid(x W_xr + h W_hr + b_r)          u = sigmoid(x W_xu + h W_hu + b_u)
    c = tanh   (x W_xc + r * (h W_hc) + b_c)    h' = (1 - u) * h + u * c          out = h' W_out + b_out

A subclass provides ``_specs(hidden)``, ``step_planes(x, h, v) -> (h', head)`` (the mean, or the softmax of ``out``) and
the attributes ``input_dim``, ``action_dim``, ``hidden_dim``, ``hidden_nonlinearity``, ``_state_include_action``.
"""
import numpy as np
import torch

from rllab_amd.core.parameterized import Param

tanh = torch.tanh
GATES = ("r", "u", "c")
KERNEL_HIDDEN = (32, 64)          # the hidden widths the recurrent rollouts are built for (narrower: zero padding)
_NO_HIDDEN_AXIS = ("output.b", "output_log_std.param")


def gru_param_specs(input_dim, hidden, action_dim, learn_std=True, log_std_row=True):
    """[(name, shape, trainable, regularizable)] in the reference's flat order (GRULayer's add_param calls,
    network.py:132-145, with hidden_init_trainable=False; the output DenseLayer; the log-std ParamLayer).
    ``log_std_row=False``: without the last row -- the GRU of a CategoricalGRUPolicy, whose output layer feeds a softmax."""
    specs = [("h0", (hidden,), False, False)]
    for g in GATES:
        specs += [("W_x" + g, (input_dim, hidden), True, True), ("W_h" + g, (hidden, hidden), True, True),
                  ("b_" + g, (hidden,), True, False)]
    specs += [("output.W", (hidden, action_dim), True, True), ("output.b", (action_dim,), True, False)]
    if log_std_row:
        specs.append(("output_log_std.param", (action_dim,), bool(learn_std), True))
    return specs


class GRUPolicyBase(object):
    # FiniteDifferenceHvp (the reference's recurrent example runs it with base_eps = 1e-5) differences two gradients at
    # theta +- eps x with eps = base_eps / |theta| ~ 1e-6.  In the parameters' float32 the shift of an entry is a few ulps of
    # that entry and the difference of the two gradients is mostly rounding: the same update on the CPU gained 169 in
    # AverageReturn over ten iterations in float32 against 399 in float64 (GaussianGRUPolicy on Cartpole).  So the two
    # shifted gradients of a GRU policy are evaluated in float64 (dist_info_planes runs in the dtype of the vector it is
    # given); parameters, loss, gradient and line search stay float32.
    fd_hvp_dtype = torch.float64

    def _build_params(self):
        """Create ``_params`` / ``_by_name`` from ``_specs(hidden_dim)`` and return the initial flat float32 numpy vector
        (host-side init with np.random, so a CPU yardstick and the GPU share theta under a seed)."""
        self._params, off = [], 0
        for name, shape, trainable, regularizable in self._specs(self.hidden_dim):
            p = Param(name, shape, off, trainable=trainable, regularizable=regularizable)
            p._owner = self
            off += p.size
            self._params.append(p)
        self._by_name = {p.name: p for p in self._params}
        flat = np.zeros(off, dtype=np.float32)
        for p in self._params:
            if len(p.shape) == 2:
                bound = np.sqrt(6.0 / (p.shape[0] + p.shape[1]))
                flat[p.offset:p.offset + p.size] = np.random.uniform(-bound, bound, size=p.shape).reshape(-1)
        return flat

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
                elif name not in _NO_HIDDEN_AXIS:
                    v[name] = zp(v[name], (0, pad))
        return v

    def _act(self, z):
        return z if self.hidden_nonlinearity is None else self.hidden_nonlinearity(z)

    def gru_planes(self, x, h, v):
        """One GRU step on planes: x [DI, N], h [H, N] -> (h' [H, N], h' W_out + b_out [Da, N]), ``v`` from ``_views``."""
        r = torch.sigmoid(v["W_xr"].t() @ x + v["W_hr"].t() @ h + v["b_r"][:, None])
        u = torch.sigmoid(v["W_xu"].t() @ x + v["W_hu"].t() @ h + v["b_u"][:, None])
        c = self._act(v["W_xc"].t() @ x + r * (v["W_hc"].t() @ h) + v["b_c"][:, None])
        h = (1 - u) * h + u * c
        return h, v["output.W"].t() @ h + v["output.b"][:, None]

    def _scan_planes(self, obs, actions, start, flat=None):
        """obs [Do, T, N], actions [Da, T, N], start [T, N] bool (a path begins at (t, n)) -> (head [Da, T, N], views): the
        scan over t of every env column of ``step_planes``, with ``h`` put back to ``h0`` and ``prev_action`` to 0 wherever
        a path starts (``prev_action[t] = actions[t-1]`` elsewhere; row 0 starts a path in every column).  In the dtype of
        ``flat``, differentiable twice."""
        flat = self.flat_params if flat is None else flat
        dt = flat.dtype
        v = self._views(flat)
        obs, actions = obs.to(dt), actions.to(dt)
        T, N = obs.shape[1], obs.shape[2]
        start = torch.as_tensor(start, device=obs.device).bool()
        h0 = v["h0"][:, None]
        h = h0.expand(h0.shape[0], N)
        zeros = torch.zeros((self.action_dim, N), dtype=dt, device=obs.device)
        heads = []
        for t in range(T):
            if t > 0:
                st = start[t][None, :]
                h = torch.where(st, h0, h)
            x = obs[:, t]
            if self._state_include_action:
                pa = zeros if t == 0 else torch.where(st, zeros, actions[:, t - 1])
                x = torch.cat([x, pa], dim=0)
            h, head = self.step_planes(x, h, v)
            heads.append(head)
        return torch.stack(heads, dim=1), v

    def _sym_planes(self, obs_var, state_info_vars):
        """The reference's [N, T, .] inputs (one padded path per row, ``state_info_vars["prev_action"]``) as the
        (obs [Do, T, N], actions [Da, T, N], start [T, N]) that the scan takes."""
        dt, dev = self.flat_params.dtype, self.flat_params.device
        obs = torch.as_tensor(obs_var, dtype=dt, device=dev)
        n, T = obs.shape[0], obs.shape[1]
        obs = obs.reshape(n, T, -1).permute(2, 1, 0)
        start = torch.zeros((T, n), dtype=torch.bool, device=dev)
        start[0] = True
        if self._state_include_action:
            prev = torch.as_tensor(state_info_vars["prev_action"], dtype=dt, device=dev).reshape(n, T, -1).permute(2, 1, 0)
            # the scan takes the actions themselves: actions[t - 1] = prev_action[t]
            actions = torch.cat([prev[:, 1:], torch.zeros_like(prev[:, :1])], dim=1)
        else:
            actions = torch.zeros((self.action_dim, T, n), dtype=dt, device=dev)
        return obs, actions, start

    # -- host stepping state ------------------------------------------------------------------------------------------
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

    def get_action(self, observation):
        actions, agent_infos = self.get_actions([observation])
        return actions[0], {k: v[0] for k, v in agent_infos.items()}

    # -- what the recurrent rollout kernels read ------------------------------------------------------------------------
    def why_no_kernel_layout(self):
        """Why the UPDATE of this policy runs through torch autograd (algos/npo.py::log_update_path)."""
        return "recurrent policy (no BPTT kernels)"

    @property
    def kernel_hidden(self):
        """The hidden width the kernel runs this policy at: the next of 32 / 64."""
        return next((H for H in KERNEL_HIDDEN if self.hidden_dim <= H), None)

    @property
    def sensor_rows(self):
        """``(full_obs_dim, ids)`` of a policy built on kept observation rows (``EnvSpec.sensor_rows``), else None."""
        return getattr(self, "_sensor_rows", None)

    @property
    def kernel_obs_dim(self):
        """The observation width the kernels run this policy at: the env's full observation under ``sensor_rows``."""
        return self.obs_dim if self.sensor_rows is None else self.sensor_rows[0]

    @property
    def kernel_layout_is_flat(self):
        """True when the kernels' parameter vector IS the flat one: no hidden unit padded, no observation row occluded."""
        return self.hidden_dim == self.kernel_hidden and self.sensor_rows is None

    def pad_index(self):
        """Index of every parameter inside the kernel's vector: the same order with the hidden axis zero-padded to
        ``kernel_hidden``.  Exact: a padded unit has zero weights and bias, so c = tanh(0) = 0, it starts at h0 = 0 and
        h' = (1 - u) 0 + u 0 stays 0; its outgoing weights are 0.
        Under ``sensor_rows = (full_obs_dim, ids)`` the input axis of W_x* is laid out on the env's full observation too:
        kept row j goes to row ids[j], the previous-action rows go behind ``full_obs_dim``, the rows of the occluded
        observations stay zero -- products with 0, in the kernel's input-index order the kept rows' sums are unchanged."""
        H, Hp = self.hidden_dim, self.kernel_hidden
        sensor = self.sensor_rows
        idx, off = [], 0
        for name, shape, _, _ in self._specs(H):
            rows = 1 if len(shape) == 1 else shape[0]
            cols = shape[-1]
            row_at = np.arange(rows)
            if name in _NO_HIDDEN_AXIS:
                rows_p, cols_p = 1, cols
            elif name == "output.W":
                rows_p, cols_p = Hp, cols
            elif name.startswith("W_h"):
                rows_p, cols_p = Hp, Hp
            else:                                   # h0, b_*: one row; W_x*: one row per input
                rows_p, cols_p = rows, Hp
                if sensor is not None and name.startswith("W_x"):
                    kept = len(sensor[1])
                    rows_p = rows - kept + sensor[0]
                    row_at = np.concatenate([np.asarray(sensor[1], dtype=np.int64), sensor[0] + np.arange(rows - kept)])
            r, c = np.meshgrid(row_at, np.arange(cols), indexing="ij")
            idx.append((off + r * cols_p + c).reshape(-1))
            off += rows_p * cols_p
        return np.concatenate(idx), off

    def pack_rows(self, xs):
        """Parameter ROWS [n_cand, P] (float32, device) -> kernel-layout rows [n_cand, P_pad], row c what
        ``rollout_layout()`` holds after ``set_param_values(xs[c])``: zeros at the padded hidden units and the occluded
        observation rows (a population of
        candidates: ``HipVecEnv.rollout_population_recurrent``)."""
        if self.kernel_layout_is_flat:
            return xs
        idx, size = self.pad_index()
        out = torch.zeros((xs.shape[0], size), dtype=xs.dtype, device=xs.device)
        out.index_copy_(1, torch.as_tensor(idx, dtype=torch.long, device=xs.device), xs)
        return out

    def rollout_layout(self):
        """The kernel's parameter vector (float32, device, refreshed when the parameters have moved), or None when the
        recurrent rollout kernel does not run this policy (``why_no_rollout_kernel()`` says why)."""
        if self.why_no_rollout_kernel() is not None:
            return None
        if self.kernel_layout_is_flat:
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
