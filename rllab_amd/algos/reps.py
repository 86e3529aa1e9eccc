"""Relative Entropy Policy Search (API and control flow of rllab/algos/reps.py:13-342).

Per iteration: minimise the dual  g(eta, v)  over  x = [eta, v]  with L-BFGS-B (eta >= 0), then fit the
policy by L-BFGS to  -mean_b(w_b log p_theta(a_b|o_b)),  w_b = exp(delta_b / eta - max delta / eta),
delta_b = r_b + (phi(s'_b) - phi(s_b)) . v  (reference :102-112, :174-184).

The functions below are the DEFINITION on the dense ``[T, N]`` planes of a ``Trajectories`` batch (float64
torch, any device): features (:207-211), feature differences (:228-238, "next sample" = next valid step of the
same path, else the zero row the reference appends per path), dual, gradient, weights.  They are the fallback
for any batch or policy the kernels do not take and what the kernels are tested against.  On a policy with
``fused_ops()`` the dual runs through rl_reps_dual (one read of the batch per evaluation, d + 4 doubles to the
host), the weights through rl_reps_weights, the policy objective and its gradient through
rl_policy_grad_loss(vpg != 0) with the weights in the ``advantages`` slot.

    J. Peters, K. Mulling, Y. Altun, "Relative Entropy Policy Search", AAAI 2010.
"""
import ctypes

import numpy as np
import scipy.optimize
import torch

import rllab_amd.misc.logger as logger
from rllab_amd.algos.batch_polopt import BatchPolopt
from rllab_amd.algos.npo import log_update_path, npo_inputs
from rllab_amd.core.serializable import Serializable
from rllab_amd.misc.device_io import read_async
from rllab_amd.optimizers.lbfgs_optimizer import value_and_grad
from rllab_amd.policies.update_batch import GaussianBatch, is_categorical, new_dist, old_dist
from rllab_amd.sampler import dist as D

MAX_KERNEL_OBS_DIM = 30      # rl_reps_dual: 2 * obs_dim + 4 <= 64


def reps_features(obs, tin):
    """[d, T, N] float64 features of every sample (reps.py:207-211): clip(o), clip(o)^2, al, al^2, al^3, 1 with
    al = (step inside its path) / 100."""
    o = torch.clamp(obs.to(torch.float64), -10.0, 10.0)
    al = (tin.to(torch.float64) / 100.0).unsqueeze(0)
    return torch.cat([o, o ** 2, al, al ** 2, al ** 3, torch.ones_like(al)], dim=0)


def reps_feat_diff(obs, tin, dones, valid):
    """[d, T, N] float64: phi(next sample of the same path) - phi(sample); the next sample of (t, n) is (t + 1, n)
    unless the path ends there (done flag, last recorded step, or (t + 1, n) cut from the batch): then zeros
    (reps.py:228-238)."""
    phi = reps_features(obs, tin)
    link = (dones[:-1] == 0) & valid[1:].bool()
    nxt = torch.zeros_like(phi)
    nxt[:, :-1] = phi[:, 1:] * link.unsqueeze(0).to(phi.dtype)
    return nxt - phi


def reps_dual_sums(eta, v, rewards, feat_diff, valid):
    """(m, S, S_delta, count, S_phi [d], delta [T, N], e [T, N]) over the valid samples, float64 tensors:
    m = max delta / eta, e = exp(delta / eta - m), S = sum e, S_delta = sum e delta, S_phi = sum e feat_diff."""
    vt = torch.as_tensor(np.asarray(v, dtype=np.float64), device=rewards.device)
    ok = valid.bool()
    delta = rewards.to(torch.float64) + (feat_diff * vt.reshape(-1, 1, 1)).sum(dim=0)        # reps.py:102
    z = delta / eta
    m = z[ok].max()
    e = torch.where(ok, torch.exp(z - m), torch.zeros_like(z))
    return m, e.sum(), (e * delta).sum(), ok.sum().to(torch.float64), (feat_diff * e.unsqueeze(0)).sum(dim=(1, 2)), delta, e


def dual_from_sums(eta, sums, epsilon, L2_reg_dual):
    """Dual (reps.py:174-184) and its gradient with respect to [eta, v] (:187) from
    sums = [m, S, S_delta, count, S_phi...] (host float64)."""
    m, S, S_delta, count = (np.float64(x) for x in sums[:4])
    eta = np.float64(eta)
    lme = np.log(S / count) + m                                  # log mean exp(delta / eta)
    dual = eta * epsilon + eta * lme + L2_reg_dual * (eta ** 2 + 1.0 / eta ** 2)
    d_eta = epsilon + lme - S_delta / (eta * S) + L2_reg_dual * (2.0 * eta - 2.0 / eta ** 3)
    grad = np.concatenate([[d_eta], np.asarray(sums[4:], dtype=np.float64) / S])
    return float(dual), grad


def reps_dual(eta, v, rewards, feat_diff, valid, epsilon, L2_reg_dual=0.0):
    """The definition: (dual, gradient over [eta, v]) in float64."""
    m, S, S_delta, count, S_phi, _, _ = reps_dual_sums(eta, v, rewards, feat_diff, valid)
    sums = torch.cat([torch.stack([m, S, S_delta, count]), S_phi]).cpu().numpy()
    return dual_from_sums(float(eta), sums, epsilon, L2_reg_dual)


def reps_weights(eta, v, rewards, feat_diff, valid):
    """[T, N] float64 sample weights exp(delta / eta - max delta / eta) of the policy loss (reps.py:110-112), 0 on
    samples cut from the batch."""
    return reps_dual_sums(eta, v, rewards, feat_diff, valid)[6]


def _positive_eta(fn):
    """The dual exists for eta > 0 only; the bound of the search is eta >= 0 (reps.py:270-271).  At the bound itself the
    line search is told "worse than anything" instead of being handed the NaNs of 0 / 0."""
    def guarded(x):
        if not x[0] > 0.0:
            return np.inf, np.zeros(len(x))
        return fn(x)
    return guarded


class FusedRepsDual(object):
    """rl_reps_dual / rl_reps_weights on one batch (csrc/reps_kernels.hip)."""

    def __init__(self, traj):
        from rllab_amd import _lib
        self._lib = _lib
        self.T, self.N, self.Do = traj.T, traj.N, traj.obs_dim
        valid = traj.valid
        self.valid = valid.contiguous().view(torch.uint8) if valid.dtype == torch.bool else \
            valid.to(torch.uint8).contiguous()
        self.dones = traj.dones.contiguous() if traj.dones.dtype == torch.uint8 else \
            traj.dones.to(torch.uint8).contiguous()
        self.obs, self.rewards = traj.obs.contiguous(), traj.rewards.contiguous()
        self.tin = traj.tin.to(torch.int32).contiguous()
        dev = traj.device
        self.ws = torch.empty(_lib.lib.rl_reps_workspace_bytes(self.T, self.N), dtype=torch.uint8, device=dev)
        self.d = 2 * self.Do + 4
        self.out = torch.empty(self.d + 4, dtype=torch.float64, device=dev)

    @staticmethod
    def accepts(traj):
        return traj.obs.is_cuda and traj.obs_dim <= MAX_KERNEL_OBS_DIM and traj.valid is not None and \
            traj.tin is not None and traj.obs.dtype == torch.float32 and traj.rewards.dtype == torch.float32

    def _v(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert v.size == self.d
        return v, v.ctypes.data_as(ctypes.c_void_p)

    def launch(self, eta, v):
        """Enqueue one evaluation; the sums [m, S, S_delta, count, S_phi] stay in ``self.out`` (device)."""
        _lib = self._lib
        v, vp = self._v(v)
        _lib.check(_lib.lib.rl_reps_dual(self.T, self.N, self.Do, _lib.ptr(self.obs), _lib.ptr(self.rewards),
                                         _lib.ptr(self.tin), _lib.ptr(self.dones), _lib.ptr(self.valid), float(eta), vp,
                                         _lib.ptr(self.ws), self.ws.numel(), _lib.ptr(self.out), _lib.stream_ptr()),
                   "rl_reps_dual")
        return self.out

    def sums(self, eta, v):
        """The d + 4 doubles of one evaluation on the host (pinned read; nothing batch-sized leaves the device)."""
        return read_async(self.launch(eta, v)).get()

    def weights(self, eta, v):
        """[T, N] float32 weights at (eta, v); evaluates the dual there first (its maximum is the weights' reference)."""
        _lib = self._lib
        out = self.launch(eta, v)
        w = torch.empty((self.T, self.N), dtype=torch.float32, device=self.obs.device)
        v, vp = self._v(v)
        _lib.check(_lib.lib.rl_reps_weights(self.T, self.N, self.Do, _lib.ptr(self.obs), _lib.ptr(self.rewards),
                                            _lib.ptr(self.tin), _lib.ptr(self.dones), _lib.ptr(self.valid), float(eta),
                                            vp, _lib.ptr(out), _lib.ptr(w), _lib.stream_ptr()), "rl_reps_weights")
        return w


class REPS(BatchPolopt, Serializable):
    """
    :param epsilon: Max KL divergence between new policy and old policy.
    :param L2_reg_dual: Dual regularization
    :param L2_reg_loss: Loss regularization
    :param max_opt_itr: Maximum number of batch optimization iterations.
    :param optimizer: must support the interface of scipy.optimize.fmin_l_bfgs_b.
    """

    def __init__(self, epsilon=0.5, L2_reg_dual=0., L2_reg_loss=0., max_opt_itr=50,
                 optimizer=scipy.optimize.fmin_l_bfgs_b, **kwargs):
        Serializable.quick_init(self, locals())
        super(REPS, self).__init__(**kwargs)
        self.epsilon = epsilon
        self.L2_reg_dual = L2_reg_dual
        self.L2_reg_loss = L2_reg_loss
        self.max_opt_itr = max_opt_itr
        self.optimizer = optimizer
        self.opt_info = None

    def init_opt(self):
        if self.policy.recurrent:
            raise NotImplementedError("recurrent policies are outside the hot path built here")
        if D.is_distributed():
            raise NotImplementedError("REPS on env shards: the dual's log-sum-exp is not folded across ranks")
        if is_categorical(self.policy):
            raise NotImplementedError("REPS on a categorical policy: its weighted maximum-likelihood fit runs on the "
                                      "Gaussian log-likelihood kernels only")
        policy = self.policy
        dist = policy.distribution
        # Init dual param values (reps.py:55-57)
        self.param_eta = 15.
        self.param_v = np.random.rand(self.env.observation_space.flat_dim * 2 + 4)
        reg_params = policy.get_params(regularizable=True)
        l2 = float(self.L2_reg_loss)

        def regulariser(flat):         # reps.py:115-118
            if l2 == 0.0 or not reg_params:
                return 0.0
            return l2 * sum((p.view(flat) ** 2).mean() for p in reg_params) / len(reg_params)

        def loss(flat, *inputs):                                                 # reps.py:110-118
            b = GaussianBatch._make(inputs)                                      # (the sample weights ride as ``advantages``)
            logli = dist.log_likelihood_sym(b.actions, new_dist(policy, b, flat), axis=0)
            return -(logli * b.advantages * b.weights).sum() * b.inv_count.to(logli.dtype) + regulariser(flat)

        def f_kl(inputs):                                                        # reps.py:155
            b = GaussianBatch._make(inputs)
            with torch.no_grad():
                kl = dist.kl_sym(old_dist(b), new_dist(policy, b), axis=0)
                return float((kl * b.weights).sum().to(torch.float64) * b.inv_count)

        fused = policy.fused_ops() if hasattr(policy, "fused_ops") and getattr(self, "use_fused", True) else None
        log_update_path(policy, fused)
        self._fused = fused
        self.opt_info = dict(f_loss=loss, f_kl=f_kl, regulariser=regulariser)

    # -- the two objectives as (value, gradient) pairs in float64 ------------------------------------------------
    def _dual_fn(self, traj):
        """x = [eta, v] -> (dual, gradient); on the kernels when they take the batch, else the definition."""
        eps, l2 = self.epsilon, self.L2_reg_dual
        if self._fused is not None and FusedRepsDual.accepts(traj):
            k = FusedRepsDual(traj)
            return k, _positive_eta(lambda x: dual_from_sums(float(x[0]), k.sums(x[0], x[1:]), eps, l2))
        fd = reps_feat_diff(traj.obs, traj.tin, traj.dones, traj.valid)
        return None, _positive_eta(lambda x: reps_dual(float(x[0]), x[1:], traj.rewards, fd, traj.valid, eps, l2))

    def _policy_fn(self, inputs):
        """flat trainable parameters -> (loss, gradient) at the policy, which is left at those parameters."""
        policy, fused = self.policy, self._fused
        use = fused is not None and fused.accepts(inputs)
        reg = self.opt_info["regulariser"]
        l2 = float(self.L2_reg_loss)

        def reg_value_grad():
            flat = policy.flat_params.detach().to(torch.float64).requires_grad_(True)
            r = reg(flat)
            (g,) = torch.autograd.grad(r, flat)
            idx = policy._flat_index(trainable=True)
            return float(r), (g if idx is None else g[idx]).cpu().numpy()

        def fn(params):
            policy.set_param_values(params, trainable=True)
            if not use:
                return value_and_grad(self.opt_info["f_loss"], policy, inputs)
            val, g = fused.value_and_grad(inputs, vpg=True)
            if l2 != 0.0:
                rv, rg = reg_value_grad()
                val, g = val + rv, g + rg
            return val, g
        return fn

    def optimize_policy(self, itr, samples_data):
        traj = samples_data["_traj"]
        if traj.tin is None:
            traj.tin = traj.time_in_path().to(torch.int32)
        if traj.valid is None:
            traj.valid = torch.ones((traj.T, traj.N), dtype=torch.bool, device=traj.device)

        #################
        # Optimize dual #
        #################
        kern, eval_dual = self._dual_fn(traj)
        x0 = np.hstack([self.param_eta, self.param_v]).astype(np.float64)
        # eta > 0, v unrestricted (reps.py:270-271)
        bounds = [(-np.inf, np.inf) for _ in x0]
        bounds[0] = (0., np.inf)
        logger.log('optimizing dual')
        eta_before = x0[0]
        dual_before = eval_dual(x0)[0]
        params_ast, _, _ = self.optimizer(func=eval_dual, x0=x0, bounds=bounds, maxiter=self.max_opt_itr, disp=0)
        dual_after = eval_dual(params_ast)[0]
        self.param_eta = float(params_ast[0])
        self.param_v = np.array(params_ast[1:], dtype=np.float64)

        ###################
        # Optimize policy #
        ###################
        if kern is not None:
            wts = kern.weights(self.param_eta, self.param_v)
        else:
            fd = reps_feat_diff(traj.obs, traj.tin, traj.dones, traj.valid)
            wts = reps_weights(self.param_eta, self.param_v, traj.rewards, fd, traj.valid).to(traj.rewards.dtype)
        inputs = npo_inputs(self.policy, samples_data)._replace(advantages=wts.reshape(traj.B))
        eval_loss = self._policy_fn(inputs)
        cur_params = np.asarray(self.policy.get_param_values(trainable=True), dtype=np.float64)
        loss_before = eval_loss(cur_params)[0]
        logger.log('optimizing policy')
        params_ast, _, _ = self.optimizer(func=eval_loss, x0=cur_params, disp=0, maxiter=self.max_opt_itr)
        loss_after = eval_loss(params_ast)[0]
        fused = self._fused
        if fused is not None and fused.accepts(inputs):
            mean_kl = fused.loss_stats_host(inputs)[1]
            fused.release()
        else:
            mean_kl = self.opt_info["f_kl"](inputs)

        logger.log('eta %f -> %f' % (eta_before, self.param_eta))
        logger.record_tabular("LossBefore", loss_before)
        logger.record_tabular("LossAfter", loss_after)
        logger.record_tabular('DualBefore', dual_before)
        logger.record_tabular('DualAfter', dual_after)
        logger.record_tabular('MeanKL', mean_kl)

    def get_itr_snapshot(self, itr, samples_data):
        return dict(itr=itr, policy=self.policy, baseline=self.baseline, env=self.env)
