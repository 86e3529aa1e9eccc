"""Natural Policy Optimization (API of rllab/algos/npo.py:10-132).

``init_opt`` hands the optimizer two closures instead of Theano expressions:
    surr_loss(theta) = - sum_b w_b * lr_b * adv_b / W      lr = p_theta(a|o) / p_old(a|o)
    mean_kl(theta)   =   sum_b w_b * KL(old_b || theta) / W
(reference :72-82; w = 0/1 validity weights of the dense batch, W = global number
of valid samples, so a sum all-reduce over env shards yields the global mean).
The inputs are the policy's update batch (rllab_amd/policies/update_batch.py: the four signatures and their order).  All
per-sample tensors are "planes" with the sample axis LAST (obs [Do, B], actions [Da, B], ...).
"""
import os

import torch

import rllab_amd.misc.logger as logger
from rllab_amd.algos.batch_polopt import BatchPolopt
from rllab_amd.policies.update_batch import is_categorical, new_dist, old_dist, signature_of
from rllab_amd.sampler import dist as D


def npo_inputs(policy, samples_data):
    """Build the optimizer input tuple (the policy's signature of policies/update_batch.py) from a processed dense batch."""
    traj = samples_data["_traj"]
    B = traj.B
    sig = signature_of(policy)
    if getattr(traj, "count", None) is not None:
        # process_samples already read the global number of valid samples (rl_sample_stats): no second
        # reduction + blocking read for 1 / W
        cnt = torch.tensor(float(traj.count), dtype=torch.float64)
    else:
        cnt = D.all_reduce_sum_(traj.valid.reshape(B).to(torch.float64).sum())
    if sig.has_start:
        # a recurrent policy: the planes stay [., T, N] -- its forward pass is a scan over t of every env column -- and the
        # path starts ride along
        old = (traj.means,)
        if "old_log_std" in sig._fields:
            if traj.log_std_planes is not None:
                raise NotImplementedError("a recurrent batch with per-sample log_std planes")
            old += (traj.log_std.reshape(-1, 1, 1),)
        return sig(traj.obs, traj.actions, traj.advantages, *old, (traj.tin == 0), traj.valid.to(torch.float32), (1.0 / cnt))
    # the MLP families: flat [., B] planes (a categorical batch: one-hot planes, the recorded probabilities as ``means``)
    old = (traj.means.reshape(traj.act_dim, B),)
    if "old_log_std" in sig._fields:
        old += (traj.log_std.reshape(-1, 1) if traj.log_std_planes is None else traj.log_std_planes.reshape(traj.act_dim, B),)
    return sig(traj.obs.reshape(traj.obs_dim, B), traj.actions.reshape(traj.act_dim, B), traj.advantages.reshape(B), *old,
               traj.valid.reshape(B).to(torch.float32), (1.0 / cnt))


def log_update_path(policy, fused, why=None):
    """One log line naming where loss / gradient / Fisher-vector products of the update run, and why when it is not
    the HIP kernels (the autograd path costs 10-20x at the batch sizes this engine samples)."""
    if fused is not None:
        logger.log("update path: HIP kernels (%s)" % type(fused).__name__)
        return
    if why is None and hasattr(policy, "why_no_kernel_layout"):
        why = policy.why_no_kernel_layout()
    if why is None and getattr(policy, "recurrent", False) and getattr(policy, "bptt_kernels", False):
        # nothing about the policy keeps it off its kernels: the caller is not the optimizer they are built for
        why = "the recurrent kernels serve ConjugateGradientOptimizer (TRPO, TNPG)"
    logger.log("update path: torch autograd%s" % ("" if why is None else " -- " + why))


def check_categorical_supported(policy):
    """What the categorical path does not do, said in a sentence (called by the algorithms' ``init_opt``)."""
    if getattr(policy, "num_seq_inputs", 1) != 1:
        raise NotImplementedError("CategoricalMLPPolicy(num_seq_inputs > 1): the batch planes hold one observation per "
                                  "sample")
    if D.is_distributed():
        raise NotImplementedError("a categorical policy is trained in one process on one GPU (not sharded over ranks)")


def check_recurrent_supported(policy, optimizer=None):
    """What the recurrent path does not do, said in a sentence (called by the algorithms' ``init_opt``)."""
    if D.is_distributed():
        raise NotImplementedError("a recurrent policy is trained in one process on one GPU (not sharded over ranks)")
    if getattr(optimizer, "_subsample_factor", 1.0) < 1:
        raise NotImplementedError("ConjugateGradientOptimizer(subsample_factor < 1) with a recurrent policy: a subsample "
                                  "must keep whole paths, the optimizer draws single samples")


def pick_optimizer(optimizer, optimizer_args, default_cls, **default_args):
    """The optimizer an NPO variant runs with: the one handed in, else ``default_cls`` built from the
    variant's defaults overridden by ``optimizer_args``."""
    if optimizer is not None:
        return optimizer
    return default_cls(**dict(default_args, **(optimizer_args or {})))


class NPO(BatchPolopt):
    def __init__(self, optimizer=None, optimizer_args=None, step_size=0.01,
                 truncate_local_is_ratio=None, **kwargs):
        if optimizer is None:
            from rllab_amd.optimizers.penalty_lbfgs_optimizer import PenaltyLbfgsOptimizer
            optimizer = pick_optimizer(None, optimizer_args, PenaltyLbfgsOptimizer)   # reference default (npo.py:27-30)
        self.optimizer = optimizer
        self.step_size = step_size
        self.truncate_local_is_ratio = truncate_local_is_ratio
        super(NPO, self).__init__(**kwargs)

    def init_opt(self):
        policy = self.policy
        dist = policy.distribution
        trunc = self.truncate_local_is_ratio
        sig = signature_of(policy)
        if policy.recurrent:
            check_recurrent_supported(policy, self.optimizer)
        if is_categorical(policy):
            check_categorical_supported(policy)

        # (recurrent: the reference's masked means over [paths, max_path_length], npo.py:72-79 with ``valids``, on the dense
        # planes)
        def surr_loss(flat, *inputs):
            b = sig._make(inputs)
            lr = dist.likelihood_ratio_sym(b.actions, old_dist(b), new_dist(policy, b, flat), axis=0)
            if trunc is not None:
                lr = torch.clamp(lr, max=trunc)
            return -(lr * b.advantages * b.weights).sum() * b.inv_count.to(lr.dtype)

        def mean_kl(flat, *inputs):
            b = sig._make(inputs)
            kl = dist.kl_sym(old_dist(b), new_dist(policy, b, flat), axis=0)
            return (kl * b.weights).sum() * b.inv_count.to(kl.dtype)

        fused = None
        trunc_why = None if trunc is None else \
            "truncate_local_is_ratio is set (the kernels evaluate the plain likelihood ratio)"
        if policy.recurrent:
            # GaussianGRUPolicy(bptt_kernels=True) under a ConjugateGradientOptimizer: policies/fused_gru_ops.py
            from rllab_amd.optimizers.conjugate_gradient_optimizer import ConjugateGradientOptimizer
            why = None
            if getattr(policy, "bptt_kernels", False) and hasattr(policy, "fused_ops"):
                why = trunc_why
                if trunc is None and isinstance(self.optimizer, ConjugateGradientOptimizer) and getattr(self, "use_fused", True):
                    fused = policy.fused_ops()
            log_update_path(policy, fused, why)
        else:
            if trunc is None and hasattr(policy, "fused_ops") and getattr(self, "use_fused", True):
                fused = policy.fused_ops()
            log_update_path(policy, fused, trunc_why)
        self.optimizer.update_opt(loss=surr_loss, target=policy, leq_constraint=(mean_kl, self.step_size),
                                  inputs=None, constraint_name="mean_kl", fused=fused)
        return dict()

    def prefetch_update(self, samples_data):
        """Called by ``process_samples`` once the advantages are on the device: hands the optimizer its inputs early so
        that its first pass runs while the host logs (optimizers/conjugate_gradient_optimizer.py::prefetch)."""
        self._prefetched = None
        if not hasattr(self.optimizer, "prefetch") or not getattr(self, "prefetch_update_enabled", True) or \
                os.environ.get("RLLAB_UPDATE_PREFETCH", "1")[:1] == "0":       # (A/B timing)
            return
        values = npo_inputs(self.policy, samples_data)
        self._prefetched = (samples_data, values)
        self.optimizer.prefetch(values)

    def optimize_policy(self, itr, samples_data):
        pre, self._prefetched = getattr(self, "_prefetched", None), None
        all_input_values = pre[1] if pre is not None and pre[0] is samples_data else npo_inputs(self.policy, samples_data)
        if getattr(self.optimizer, "reports_before_values", False):
            # (train_iteration's hook: what to enqueue behind the update before its outcome is read -- the next rollout)
            self.optimizer._after_enqueue = getattr(self, "_after_update_enqueued", None)
            try:
                self.optimizer.optimize(all_input_values)
            finally:
                self.optimizer._after_enqueue = None
            loss_before, mean_kl_before = self.optimizer.last_before
        else:
            loss_before = self.optimizer.loss(all_input_values)
            mean_kl_before = self.optimizer.constraint_val(all_input_values)
            self.optimizer.optimize(all_input_values)
        mean_kl = self.optimizer.constraint_val(all_input_values)
        loss_after = self.optimizer.loss(all_input_values)
        logger.record_tabular('LossBefore', loss_before)
        logger.record_tabular('LossAfter', loss_after)
        logger.record_tabular('MeanKLBefore', mean_kl_before)
        logger.record_tabular('MeanKL', mean_kl)
        logger.record_tabular('dLoss', loss_before - loss_after)
        fused = getattr(self.optimizer, "_fused", None)
        if fused is not None:
            fused.release()   # drop the cached batch descriptor (it keeps the batch tensors alive)
        return dict()

    def get_itr_snapshot(self, itr, samples_data):
        return dict(itr=itr, policy=self.policy, baseline=self.baseline, env=self.env)
