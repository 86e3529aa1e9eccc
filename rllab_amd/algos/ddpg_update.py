"""The fused DDPG update: rl_ddpg_update (csrc/ddpg_kernels.hip) behind the policy / Q-function objects.

``FusedDDPGUpdate`` owns the kernel's state buffer -- parameters, targets, Adam moments and step counts of both nets in
the kernel's padded layout -- and launches K updates on a ``DeviceReplayPool`` in ONE call of the binding.  There is no
second path: a shape the kernel does not run is refused with a sentence (``ddpg_why_unsupported``).

Layout of the state buffer (float32): planes theta, targets, m, v, scratch of P entries each, then two int32 step
counts (Q, policy).  A plane is [policy | Q]; a net is W0[in][H0p] b0 W1[in1][H1p] b1 W2[H1p][out] b2 with the hidden
widths padded to 32 or 64 (zeros) and Q's W1 holding H0p hidden rows followed by the action rows.  ``net_index`` maps the
objects' flat vectors (unpadded, the reference's order) into a plane.
"""
import ctypes

import numpy as np
import torch

from rllab_amd import _lib

MAX_OBS, MAX_ACT, MAX_HIDDEN, MAX_BATCH, MAX_UPDATES = 32, 8, 64, 128, 16384
METHODS = {"adam": _lib.DDPG_ADAM, "sgd": _lib.DDPG_SGD}
STAT_KEYS = ("qf_loss", "policy_surr", "updates", "q", "abs_q", "y", "abs_y", "abs_q_y_diff", "samples")


def parse_update_method(update_method):
    """'adam' / 'sgd' -> the kernel's method code (rllab/algos/ddpg.py:16-22)."""
    if update_method not in METHODS:
        raise NotImplementedError("update method %r: the DDPG update kernel steps with 'adam' or 'sgd'" % (update_method,))
    return METHODS[update_method]


def pad_width(h):
    return 32 if h <= 32 else 64


def _activation_code(f, what, allowed):
    from rllab_amd.policies.gaussian_mlp_policy import is_rectify
    if f is None:
        code = _lib.ACT_IDENTITY
    elif f is torch.tanh:
        code = _lib.ACT_TANH
    elif is_rectify(f):
        code = _lib.ACT_RECTIFY
    else:
        return None, "%s is %r: the DDPG update kernel evaluates %s" % (what, getattr(f, "__name__", f), allowed)
    return code, None


def ddpg_why_unsupported(policy, qf, batch_size=32, n_updates=1):
    """One sentence naming what keeps this policy / Q-function / batch off rl_ddpg_update, or None."""
    from rllab_amd.policies.deterministic_mlp_policy import DeterministicMLPPolicy
    from rllab_amd.q_functions.continuous_mlp_q_function import ContinuousMLPQFunction
    if not isinstance(policy, DeterministicMLPPolicy):
        return "%s is not a DeterministicMLPPolicy" % type(policy).__name__
    if not isinstance(qf, ContinuousMLPQFunction):
        return "%s is not a ContinuousMLPQFunction" % type(qf).__name__
    for name, hs in (("policy", policy.hidden_sizes), ("qf", qf.hidden_sizes)):
        if len(hs) != 2:
            return "%s hidden_sizes=%r: the DDPG update kernel runs two hidden layers" % (name, tuple(hs))
        if not all(1 <= h <= MAX_HIDDEN for h in hs):
            return "%s hidden_sizes=%r: the DDPG update kernel runs hidden layers of at most %d units" % (
                name, tuple(hs), MAX_HIDDEN)
    if tuple(policy.hidden_sizes) != tuple(qf.hidden_sizes):
        return "policy hidden_sizes=%r and qf hidden_sizes=%r differ: the DDPG update kernel runs both nets at one pair " \
               "of widths" % (tuple(policy.hidden_sizes), tuple(qf.hidden_sizes))
    if policy.obs_dim != qf.obs_dim or policy.action_dim != qf.action_dim:
        return "policy and qf are built on different env specs"
    if policy.obs_dim > MAX_OBS or policy.action_dim > MAX_ACT:
        return "obs_dim %d, act_dim %d: the DDPG update kernel runs at most %d observation and %d action entries" % (
            policy.obs_dim, policy.action_dim, MAX_OBS, MAX_ACT)
    if qf.action_merge_layer != 1:
        return "action_merge_layer=%d: the DDPG update kernel merges the action in front of hidden layer 1" % \
            qf.action_merge_layer
    hp, why = _activation_code(policy.hidden_nonlinearity, "the policy's hidden_nonlinearity", "rectify or tanh")
    if why:
        return why
    hq, why = _activation_code(qf.hidden_nonlinearity, "the qf's hidden_nonlinearity", "rectify or tanh")
    if why:
        return why
    if hp != hq or hp == _lib.ACT_IDENTITY:
        return "the hidden nonlinearities of policy and qf must be the same one of rectify / tanh for the DDPG update kernel"
    op, why = _activation_code(policy.output_nonlinearity, "the policy's output_nonlinearity", "tanh or the identity")
    if why:
        return why
    if op == _lib.ACT_RECTIFY:
        return "the policy's output_nonlinearity is rectify: the DDPG update kernel evaluates tanh or the identity"
    if qf.output_nonlinearity is not None:
        return "the qf's output_nonlinearity is not None: the DDPG update kernel's Q head is linear"
    if not 1 <= int(batch_size) <= MAX_BATCH:
        return "batch_size=%d: the DDPG update kernel takes batches of 1 .. %d rows" % (batch_size, MAX_BATCH)
    if not 1 <= int(n_updates) <= MAX_UPDATES:
        return "%d updates per lock-step (n_envs * n_updates_per_sample): one launch of the DDPG update kernel runs " \
               "1 .. %d" % (n_updates, MAX_UPDATES)
    return None


def net_index(obs_dim, act_dim, hidden_sizes):
    """(idx_policy, idx_qf, P): positions inside a plane of the state buffer of every entry of the policy's / the
    Q-function's flat parameter vector (int64 numpy arrays), and the plane's length."""
    D, A = int(obs_dim), int(act_dim)
    h0, h1 = (int(h) for h in hidden_sizes)
    H0, H1 = pad_width(h0), pad_width(h1)

    idx_pi, end_pi = _net_index(D, h0, h1, H0, H1, 0, A, 0)
    idx_q, end_q = _net_index(D, h0, h1, H0, H1, A, 1, end_pi)
    return idx_pi, idx_q, end_q


def _net_index(D, h0, h1, H0, H1, merge, out, base):
    """One net: W0[D][H0] b0[H0] W1[H0 + merge][H1] b1[H1] W2[H1][out] b2[out] at offset ``base``; the real entries in
    the flat vector's order W0[D][h0] b0 W1[h0 + merge][h1] b1 W2[h1][out] b2."""
    def block(rows, cols, stride, off):
        r = np.asarray(rows, dtype=np.int64)[:, None]
        return (off + r * stride + np.arange(cols, dtype=np.int64)[None, :]).reshape(-1)
    idx, off = [], base
    idx.append(block(range(D), h0, H0, off)); off += D * H0
    idx.append(off + np.arange(h0, dtype=np.int64)); off += H0
    idx.append(block(list(range(h0)) + [H0 + k for k in range(merge)], h1, H1, off)); off += (H0 + merge) * H1
    idx.append(off + np.arange(h1, dtype=np.int64)); off += H1
    idx.append(block(range(h1), out, out, off)); off += H1 * out
    idx.append(off + np.arange(out, dtype=np.int64)); off += out
    return np.concatenate(idx), off


class FusedDDPGUpdate(object):
    """State buffer + launcher of rl_ddpg_update for one (policy, qf) pair."""

    def __init__(self, policy, qf, batch_size=32, device=None):
        why = ddpg_why_unsupported(policy, qf, batch_size)
        if why is not None:
            raise NotImplementedError("DDPG: %s" % why)
        self.obs_dim, self.act_dim = int(policy.obs_dim), int(policy.action_dim)
        self.hidden_sizes = tuple(int(h) for h in policy.hidden_sizes)
        self.hidden_activation = _activation_code(policy.hidden_nonlinearity, "", "")[0]
        self.output_activation = _activation_code(policy.output_nonlinearity, "", "")[0]
        self.batch_size = int(batch_size)
        self.device = torch.device(device) if device is not None else policy.flat_params.device
        idx_pi, idx_q, self.P = net_index(self.obs_dim, self.act_dim, self.hidden_sizes)
        self.idx_policy = torch.as_tensor(idx_pi, device=self.device)
        self.idx_qf = torch.as_tensor(idx_q, device=self.device)
        nbytes = int(_lib.lib.rl_ddpg_state_bytes(self.obs_dim, self.act_dim, *self.hidden_sizes))
        assert nbytes >= (5 * self.P + 2) * 4, (nbytes, self.P)
        self.state = torch.zeros(nbytes // 4, dtype=torch.float32, device=self.device)
        self.stats = torch.zeros(_lib.DDPG_STATS, dtype=torch.float64, device=self.device)
        self.load(policy.flat_params, qf.flat_params)

    # -- the state buffer ---------------------------------------------------------------------------------------------
    def plane(self, k):
        """View of plane k (0 theta, 1 targets, 2 Adam m, 3 Adam v)."""
        return self.state[k * self.P:(k + 1) * self.P]

    def load(self, policy_flat, qf_flat, target_policy_flat=None, target_qf_flat=None):
        """Parameters (and targets: the parameters themselves when not given) into the state; moments and step counts
        to zero."""
        self.state.zero_()
        f = lambda x: torch.as_tensor(x, device=self.device).to(torch.float32)
        for k, (p, q) in enumerate(((policy_flat, qf_flat),
                                    (policy_flat if target_policy_flat is None else target_policy_flat,
                                     qf_flat if target_qf_flat is None else target_qf_flat))):
            self.plane(k)[self.idx_policy] = f(p)
            self.plane(k)[self.idx_qf] = f(q)

    def unpack(self, k=0):
        """(policy flat vector, qf flat vector) of plane k, in the objects' own order."""
        pl = self.plane(k)
        return pl[self.idx_policy], pl[self.idx_qf]

    def step_counts(self):
        """(Q, policy) Adam step counts carried in the state (one host read)."""
        c = self.state[5 * self.P:5 * self.P + 2].view(torch.int32).cpu()
        return int(c[0]), int(c[1])

    def write_back(self, policy, qf, target_policy=None, target_qf=None):
        """The state's parameters (and targets) into the objects' flat vectors."""
        p, q = self.unpack(0)
        policy.flat_params.copy_(p)
        qf.flat_params.copy_(q)
        if target_policy is not None:
            tp, tq = self.unpack(1)
            target_policy.flat_params.copy_(tp)
            target_qf.flat_params.copy_(tq)

    # -- the launch ---------------------------------------------------------------------------------------------------
    def update(self, pool, n_updates, discount=0.99, tau=0.001, qf_learning_rate=1e-3, policy_learning_rate=1e-4,
               qf_weight_decay=0.0, policy_weight_decay=0.0, qf_method="adam", policy_method="adam", seed=0,
               update_base=0, indices=None, indices_out=None, q_out=None, y_out=None, stats=True, batch_size=None):
        """``n_updates`` updates on ``pool`` in one launch.  ``indices`` int32 [n_updates, batch] pool rows, or None: drawn
        in the kernel from (seed, update_base + u).  ``indices_out`` int32 / ``q_out`` / ``y_out`` float32
        [n_updates, batch]: optional outputs."""
        B = self.batch_size if batch_size is None else int(batch_size)
        K = int(n_updates)
        for name, t, dt in (("indices", indices, torch.int32), ("indices_out", indices_out, torch.int32),
                            ("q_out", q_out, torch.float32), ("y_out", y_out, torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != (K, B) or t.device != self.device):
                raise ValueError("%s must be a %s tensor of shape (%d, %d) on %s" % (name, dt, K, B, self.device))
        a = _lib.DdpgArgs(
            obs_dim=self.obs_dim, act_dim=self.act_dim, hidden0=self.hidden_sizes[0], hidden1=self.hidden_sizes[1],
            hidden_activation=self.hidden_activation, output_activation=self.output_activation, batch=B, n_updates=K,
            capacity=pool.capacity, size=pool.size, top=pool.top,
            qf_method=qf_method if isinstance(qf_method, int) else parse_update_method(qf_method),
            policy_method=policy_method if isinstance(policy_method, int) else parse_update_method(policy_method),
            discount=discount, tau=tau, qf_learning_rate=qf_learning_rate, policy_learning_rate=policy_learning_rate,
            qf_weight_decay=qf_weight_decay, policy_weight_decay=policy_weight_decay,
            seed=int(seed) & (2 ** 64 - 1), update_base=int(update_base) & (2 ** 64 - 1))
        p = lambda t: None if t is None else t.data_ptr()
        assert pool.obs.shape[1] == self.obs_dim and pool.act.shape[1] == self.act_dim
        a.state = p(self.state)
        a.obs, a.act, a.rew, a.term, a.next_obs, a.skip = (p(getattr(pool, n)) for n in pool.PLANES)
        a.indices, a.indices_out, a.q_out, a.y_out = p(indices), p(indices_out), p(q_out), p(y_out)
        a.stats = p(self.stats) if stats else None
        _lib.check(_lib.lib.rl_ddpg_update(ctypes.byref(a), _lib.stream_ptr()), "rl_ddpg_update")

    def read_stats(self, reset=True):
        """dict of the statistics block's sums (``STAT_KEYS``), one host read; ``reset``: zero it afterwards."""
        host = self.stats.cpu().numpy()
        if reset:
            self.stats.zero_()
        return dict(zip(STAT_KEYS, host[:len(STAT_KEYS)].tolist()))
