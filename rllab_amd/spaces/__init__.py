from rllab_amd.spaces.base import Space
from rllab_amd.spaces.box import Box
from rllab_amd.spaces.discrete import Discrete

__all__ = ["Space", "Box", "Discrete"]
