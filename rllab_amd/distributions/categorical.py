"""Categorical (mirrors rllab/distributions/categorical.py:23-87).

``dist_info`` is ``dict(prob=...)``; actions are one-hot.  ``TINY`` sits exactly where the reference has it: inside both
logarithms of the KL, in numerator and denominator of the likelihood ratio, and inside the logarithms of entropy and
log-likelihood.  The ``*_sym`` methods are the same formulas on torch tensors (autograd plays the role of the symbolic
graph); ``axis`` is the action axis: -1 for the reference's ``[B, A]`` layout, 0 for the engine's dense ``[A, B]``
planes.  The plain methods take numpy arrays in the reference's layout.
"""
import numpy as np
import torch

from rllab_amd.distributions.base import Distribution

TINY = 1e-8


def from_onehot(x_var):
    """[N, A] one-hot rows -> [N] int32 indices."""
    ret = np.zeros((len(x_var),), 'int32')
    nonzero_n, nonzero_a = np.nonzero(x_var)
    ret[nonzero_n] = nonzero_a
    return ret


class Categorical(Distribution):
    def __init__(self, dim):
        self._dim = dim

    @property
    def dim(self):
        return self._dim

    # -- torch ("symbolic") forms ---------------------------------------------------------------------------------
    def kl_sym(self, old_dist_info_vars, new_dist_info_vars, axis=-1):
        old_prob, new_prob = old_dist_info_vars["prob"], new_dist_info_vars["prob"]
        return torch.sum(old_prob * (torch.log(old_prob + TINY) - torch.log(new_prob + TINY)), dim=axis)

    def likelihood_ratio_sym(self, x_var, old_dist_info_vars, new_dist_info_vars, axis=-1):
        old_prob, new_prob = old_dist_info_vars["prob"], new_dist_info_vars["prob"]
        x = x_var.to(new_prob.dtype)
        return (torch.sum(new_prob * x, dim=axis) + TINY) / (torch.sum(old_prob * x, dim=axis) + TINY)

    def entropy_sym(self, dist_info_vars, axis=-1):
        prob = dist_info_vars["prob"]
        return -torch.sum(prob * torch.log(prob + TINY), dim=axis)

    def log_likelihood_sym(self, x_var, dist_info_vars, axis=-1):
        prob = dist_info_vars["prob"]
        return torch.log(torch.sum(prob * x_var.to(prob.dtype), dim=axis) + TINY)

    # -- numpy forms ([N, A]) ------------------------------------------------------------------------------------------
    def kl(self, old_dist_info, new_dist_info):
        old_prob, new_prob = np.asarray(old_dist_info["prob"]), np.asarray(new_dist_info["prob"])
        return np.sum(old_prob * (np.log(old_prob + TINY) - np.log(new_prob + TINY)), axis=-1)

    def likelihood_ratio(self, xs, old_dist_info, new_dist_info):
        old_prob, new_prob = np.asarray(old_dist_info["prob"]), np.asarray(new_dist_info["prob"])
        xs = np.asarray(xs, dtype=new_prob.dtype)
        return (np.sum(new_prob * xs, axis=-1) + TINY) / (np.sum(old_prob * xs, axis=-1) + TINY)

    def entropy(self, info):
        probs = np.asarray(info["prob"])
        return -np.sum(probs * np.log(probs + TINY), axis=-1)

    def log_likelihood(self, xs, dist_info):
        probs = np.asarray(dist_info["prob"])
        N = probs.shape[0]
        return np.log(probs[np.arange(N), from_onehot(np.asarray(xs))] + TINY)

    def sample(self, dist_info):
        """[N, A] probabilities -> [N, A] one-hot draws (np.random; the reference's ``sample_sym`` is a Theano multinomial)."""
        probs = np.asarray(dist_info["prob"])
        u = np.random.rand(len(probs), 1)
        idx = np.minimum((np.cumsum(probs, axis=-1) < u).sum(axis=-1), probs.shape[-1] - 1)
        out = np.zeros_like(probs)
        out[np.arange(len(probs)), idx] = 1
        return out

    @property
    def dist_info_keys(self):
        return ["prob"]
