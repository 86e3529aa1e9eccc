"""EnvSpec: the (observation space, action space) pair policies and baselines are built from
(API of rllab/envs/env_spec.py:5-25).

``sensor_rows`` (optional): ``(full_obs_dim, ids)`` when the observation space is a selection of the rows a HIP-native env
produces -- OcclusionEnv, Box2DEnv(position_only=True).  A recurrent policy lays its kernel parameters out on the full
observation from it (``GRUPolicyBase.pad_index``); None everywhere else."""
from rllab_amd.core.serializable import Serializable


class EnvSpec(Serializable):
    __slots__ = ()

    def __init__(self, observation_space, action_space, sensor_rows=None):
        Serializable.quick_init(self, locals())
        self._spaces = (observation_space, action_space)
        self._sensor_rows = None if sensor_rows is None else (int(sensor_rows[0]), tuple(int(i) for i in sensor_rows[1]))

    observation_space = property(lambda self: self._spaces[0])
    action_space = property(lambda self: self._spaces[1])
    sensor_rows = property(lambda self: self._sensor_rows)

    def __repr__(self):
        return "EnvSpec(obs=%r, act=%r)" % self._spaces
