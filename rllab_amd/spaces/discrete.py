"""Discrete: the integers {0, 1, ..., n - 1} (API of rllab/spaces/discrete.py:7-81).  Flat form: one-hot vectors of
length ``n`` (rllab/misc/special.py:36-65); ``weighted_sample`` draws an index by inverting the cumulative weights
against ONE np.random uniform (rllab/misc/special.py:10-19)."""
import numpy as np

from rllab_amd.spaces.base import Space


def weighted_sample(weights, objects):
    """Element of ``objects`` drawn with probability ``weights``: idx = sum(cumsum(weights) < u), u one np.random.rand(),
    clamped to the last index (cumulative sums that stop short of 1 by rounding)."""
    cs = np.cumsum(weights)
    idx = sum(cs < np.random.rand())
    return objects[min(idx, len(objects) - 1)]


class Discrete(Space):
    def __init__(self, n):
        self._n = int(n)

    @property
    def n(self):
        return self._n

    flat_dim = property(lambda self: self._n)
    default_value = property(lambda self: 0)

    def sample(self):
        return np.random.randint(self.n)

    def contains(self, x):
        x = np.asarray(x)
        return bool(x.shape == () and x.dtype.kind == 'i' and 0 <= x < self.n)

    def weighted_sample(self, weights):
        return weighted_sample(weights, range(self.n))

    # -- (un)flattening: index <-> one-hot --------------------------------------------------------------------------
    def flatten(self, x):
        ret = np.zeros(self.n)
        ret[x] = 1
        return ret

    def unflatten(self, x):
        return int(np.argmax(np.asarray(x)))

    def flatten_n(self, xs):
        xs = np.asarray(xs, dtype=np.int64).reshape(-1)
        ret = np.zeros((len(xs), self.n))
        ret[np.arange(len(xs)), xs] = 1
        return ret

    def unflatten_n(self, xs):
        return np.argmax(np.asarray(xs), axis=-1)

    # -- value semantics ----------------------------------------------------------------------------------------------
    def __eq__(self, other):
        return isinstance(other, Discrete) and self.n == other.n

    def __hash__(self):
        return hash(self.n)

    def __repr__(self):
        return "Discrete(%d)" % self.n
