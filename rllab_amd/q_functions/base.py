"""Q-function interface (mirrors rllab/q_functions/base.py)."""
from rllab_amd.core.parameterized import Parameterized


class QFunction(Parameterized):
    pass
