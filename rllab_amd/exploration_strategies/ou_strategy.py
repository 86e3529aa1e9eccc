"""OUStrategy (API of rllab/exploration_strategies/ou_strategy.py:10-53): Ornstein-Uhlenbeck noise on the actions of a
deterministic policy,  x <- x + theta (mu - x) + sigma N(0, 1),  action = clip(policy action + x, low, high).

The reference keeps one state vector; the lock-step collection of DDPG steps n envs at once, so the state here is one
row per env ([n, Da], created at the first vectorised call) and ``reset(mask)`` puts back the rows of the envs whose path
ended.  ``get_action`` is the reference's single-env call on numpy (np.random) with a state vector of its own."""
import numpy as np
import torch

from rllab_amd.core.serializable import Serializable
from rllab_amd.exploration_strategies.base import ExplorationStrategy
from rllab_amd.spaces.box import Box


class OUStrategy(ExplorationStrategy, Serializable):
    def __init__(self, env_spec, mu=0, theta=0.15, sigma=0.3, **kwargs):
        assert isinstance(env_spec.action_space, Box)
        assert len(env_spec.action_space.shape) == 1
        Serializable.quick_init(self, locals())
        self.mu = mu
        self.theta = theta
        self.sigma = sigma
        self.action_space = env_spec.action_space
        self.state = np.ones(self.action_space.flat_dim) * self.mu
        self.states = None            # [n, Da] device tensor of the vectorised path
        self.reset()

    def __getstate__(self):
        d = Serializable.__getstate__(self)
        d["state"] = self.state
        return d

    def __setstate__(self, d):
        Serializable.__setstate__(self, d)
        self.state = d["state"]

    def reset(self, mask=None):
        """No argument: every state back to mu (the reference's call).  ``mask`` [n] bool tensor: those env rows only."""
        if mask is None:
            self.state = np.ones(self.action_space.flat_dim) * self.mu
            if self.states is not None:
                self.states.fill_(float(self.mu))
        elif self.states is not None:
            self.states.masked_fill_(torch.as_tensor(mask, device=self.states.device).bool().unsqueeze(1), float(self.mu))

    # -- the reference's single-env face ------------------------------------------------------------------------------
    def evolve_state(self):
        x = self.state
        dx = self.theta * (self.mu - x) + self.sigma * np.random.randn(len(x))
        self.state = x + dx
        return self.state

    def get_action(self, t, observation, policy, **kwargs):
        action, _ = policy.get_action(observation)
        ou_state = self.evolve_state()
        return np.clip(action + ou_state, self.action_space.low, self.action_space.high)

    # -- n envs in lock step ------------------------------------------------------------------------------------------
    def evolve_states(self, normals):
        """One step of every row with the given N(0, 1) draws [n, Da]."""
        if self.states is None or self.states.shape != normals.shape or self.states.device != normals.device:
            self.states = torch.full_like(normals, float(self.mu))
        x = self.states
        self.states = x + (self.theta * (self.mu - x) + self.sigma * normals)
        return self.states

    def kernel_rule(self, itr, horizon, n_envs, device):
        """What rl_rollout_deterministic_mlp needs to apply this strategy inside a launch of ``horizon`` lock-steps of
        ``n_envs`` envs: the rule's code, its scalars and the bounds it clips to.  The executor keeps ``states`` [n, Da]
        as the state the launch starts from and ends on (``HipVecEnv.rollout_deterministic``)."""
        from rllab_amd import _lib
        return dict(code=_lib.EXPLORE_OU, theta=float(self.theta), mu=float(self.mu), sigma=float(self.sigma),
                    low=np.asarray(self.action_space.low, dtype=np.float32),
                    high=np.asarray(self.action_space.high, dtype=np.float32), sigma_t=None)

    def get_actions(self, t, observations, policy, normals=None, **kwargs):
        """observations [n, Do] tensor -> actions [n, Da] tensor on the same device; ``normals``: injected draws."""
        actions, _ = policy.get_actions(observations)
        if normals is None:
            normals = torch.randn(actions.shape, dtype=actions.dtype, device=actions.device)
        noise = self.evolve_states(normals.to(actions.dtype))
        low = torch.as_tensor(self.action_space.low, dtype=actions.dtype, device=actions.device)
        high = torch.as_tensor(self.action_space.high, dtype=actions.dtype, device=actions.device)
        return torch.max(torch.min(actions + noise, high), low)
