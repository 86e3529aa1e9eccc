"""RecurrentCategorical (rllab/distributions/recurrent_categorical.py:10-75): the categorical distribution on the
reference's padded ``[N, T, A]`` batches.

``Categorical``'s formulas (TINY = 1e-8 where the reference has it) already act along a chosen action axis whatever the
other axes are -- the last one by default, ``axis=0`` for the engine's dense ``[A, T, N]`` planes -- so ``kl``, ``entropy``,
``likelihood_ratio`` and every ``*_sym`` twin are inherited.  Only the numpy ``log_likelihood`` indexes rows and is
restated here for any number of leading axes.
"""
import numpy as np

from rllab_amd.distributions.categorical import TINY, Categorical


class RecurrentCategorical(Categorical):
    def log_likelihood(self, xs, dist_info):
        """one-hot xs [..., A], prob [..., A] -> [...]: log(prob of the taken action + TINY)."""
        probs = np.asarray(dist_info["prob"])
        return np.log(np.sum(probs * np.asarray(xs, dtype=probs.dtype), axis=-1) + TINY)
