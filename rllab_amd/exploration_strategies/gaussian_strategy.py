"""GaussianStrategy (API of rllab/exploration_strategies/gaussian_strategy.py:7-25): independent Gaussian noise on the
actions of a deterministic policy, its scale decaying linearly from ``max_sigma`` to ``min_sigma`` over
``decay_period`` steps."""
import numpy as np
import torch

from rllab_amd.core.serializable import Serializable
from rllab_amd.exploration_strategies.base import ExplorationStrategy
from rllab_amd.spaces.box import Box


class GaussianStrategy(ExplorationStrategy, Serializable):
    def __init__(self, env_spec, max_sigma=1.0, min_sigma=0.1, decay_period=1000000):
        assert isinstance(env_spec.action_space, Box)
        assert len(env_spec.action_space.shape) == 1
        Serializable.quick_init(self, locals())
        self._max_sigma = max_sigma
        self._min_sigma = min_sigma
        self._decay_period = decay_period
        self._action_space = env_spec.action_space

    def sigma(self, t):
        return self._max_sigma - (self._max_sigma - self._min_sigma) * min(1.0, t * 1.0 / self._decay_period)

    def get_action(self, t, observation, policy, **kwargs):
        action, agent_info = policy.get_action(observation)
        return np.clip(action + np.random.normal(size=len(action)) * self.sigma(t), self._action_space.low,
                       self._action_space.high)

    def kernel_rule(self, itr, horizon, n_envs, device):
        """What rl_rollout_deterministic_mlp needs to apply this strategy inside a launch of ``horizon`` lock-steps of
        ``n_envs`` envs that starts at ``itr``: the rule's code, the bounds it clips to and the device plane
        ``sigma_t`` [horizon] = sigma(itr + t * n_envs) rounded to float32 -- lock-step t of the launch is DDPG's
        ``itr + t * n_envs``."""
        from rllab_amd import _lib
        sigma_t = np.asarray([self.sigma(itr + t * n_envs) for t in range(int(horizon))], dtype=np.float32)
        return dict(code=_lib.EXPLORE_GAUSSIAN, theta=0.0, mu=0.0, sigma=0.0,
                    low=np.asarray(self._action_space.low, dtype=np.float32),
                    high=np.asarray(self._action_space.high, dtype=np.float32),
                    sigma_t=torch.as_tensor(sigma_t).to(device))

    def get_actions(self, t, observations, policy, normals=None, **kwargs):
        actions, _ = policy.get_actions(observations)
        if normals is None:
            normals = torch.randn(actions.shape, dtype=actions.dtype, device=actions.device)
        low = torch.as_tensor(self._action_space.low, dtype=actions.dtype, device=actions.device)
        high = torch.as_tensor(self._action_space.high, dtype=actions.dtype, device=actions.device)
        return torch.max(torch.min(actions + normals.to(actions.dtype) * self.sigma(t), high), low)
