"""Vanilla Policy Gradient (API of rllab/algos/vpg.py:11-139).

surr_obj = - mean(log p_theta(a|o) * adv); one full-batch Adam step per iteration
by default (``FirstOrderOptimizer(batch_size=None, max_epochs=1)``); logs
LossBefore / LossAfter / MeanKL / MaxKL.
"""
import torch

import rllab_amd.misc.logger as logger
from rllab_amd.algos.batch_polopt import BatchPolopt
from rllab_amd.algos.npo import check_categorical_supported, check_recurrent_supported, log_update_path, npo_inputs
from rllab_amd.core.serializable import Serializable
from rllab_amd.optimizers.first_order_optimizer import FirstOrderOptimizer
from rllab_amd.policies.update_batch import is_categorical, new_dist, old_dist, signature_of
from rllab_amd.sampler import dist as D


class VPG(BatchPolopt, Serializable):
    def __init__(self, env, policy, baseline, optimizer=None, optimizer_args=None, **kwargs):
        Serializable.quick_init(self, locals())
        if optimizer is None:
            default_args = dict(batch_size=None, max_epochs=1)
            optimizer_args = default_args if optimizer_args is None else dict(default_args, **optimizer_args)
            optimizer = FirstOrderOptimizer(**optimizer_args)
        self.optimizer = optimizer
        self.opt_info = None
        super(VPG, self).__init__(env=env, policy=policy, baseline=baseline, **kwargs)

    def init_opt(self):
        policy = self.policy
        dist = policy.distribution
        sig = signature_of(policy)
        if policy.recurrent:
            check_recurrent_supported(policy, self.optimizer)
        if is_categorical(policy):
            check_categorical_supported(policy)

        # (recurrent: the reference's masked means, vpg.py:60-75 with ``valids``, on the dense [., T, N] planes)
        def surr_obj(flat, *inputs):
            b = sig._make(inputs)
            logli = dist.log_likelihood_sym(b.actions, new_dist(policy, b, flat), axis=0)
            return -(logli * b.advantages * b.weights).sum() * b.inv_count.to(logli.dtype)

        def f_kl(inputs):
            b = sig._make(inputs)
            with torch.no_grad():
                kl = dist.kl_sym(old_dist(b), new_dist(policy, b), axis=0)
                # (the all-reduces are the identity in one process; only the Gaussian MLP family runs sharded)
                mean_kl = D.all_reduce_sum_(((kl * b.weights).sum() * b.inv_count.to(kl.dtype)).to(torch.float64))
                neg = torch.full_like(kl, -float("inf"))
                max_kl = D.all_reduce_max_(torch.where(b.weights > 0, kl, neg).max().to(torch.float64))
            return float(mean_kl), float(max_kl)

        fused = policy.fused_ops() if hasattr(policy, "fused_ops") and getattr(self, "use_fused", True) \
            and not policy.recurrent else None
        log_update_path(policy, fused)

        def fused_f_kl(inputs):                        # (HIP kernel version of the same statistic)
            s = fused.loss_stats_host(inputs)          # the evaluation's one host read (shared with loss())
            return s[1], s[3]
        # fused_loglik: surr_obj is the log-likelihood objective, not NPO's likelihood-ratio surrogate (LbfgsOptimizer asks
        # the fused object for the matching value / gradient: ERWR; the other optimizers ignore the keyword)
        self.optimizer.update_opt(surr_obj, target=policy, inputs=None, fused=fused, weighted_mean_inputs=True,
                                  fused_loglik=True)
        self.opt_info = dict(f_kl=f_kl if fused is None else fused_f_kl)

    def optimize_policy(self, itr, samples_data):
        logger.log("optimizing policy")
        inputs = npo_inputs(self.policy, samples_data)
        loss_before = None
        if not getattr(self.optimizer, "reports_before_values", False):
            loss_before = self.optimizer.loss(inputs)
        self.optimizer.optimize(inputs)
        if loss_before is None:
            before = getattr(self.optimizer, "last_before", None)
            # (a mini-batch or non-fused run has evaluated the loss up front itself and cached nothing for us)
            loss_before = before[0] if before is not None else float("nan")
        loss_after = self.optimizer.loss(inputs)
        logger.record_tabular("LossBefore", loss_before)
        logger.record_tabular("LossAfter", loss_after)
        mean_kl, max_kl = self.opt_info['f_kl'](inputs)
        logger.record_tabular('MeanKL', mean_kl)
        logger.record_tabular('MaxKL', max_kl)
        fused = getattr(self.optimizer, "_fused", None)
        if fused is not None:
            fused.release()

    def get_itr_snapshot(self, itr, samples_data):
        return dict(itr=itr, policy=self.policy, baseline=self.baseline, env=self.env)
