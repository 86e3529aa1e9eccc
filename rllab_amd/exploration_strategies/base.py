"""Exploration-strategy interface (mirrors rllab/exploration_strategies/base.py), plus the vectorised call the lock-step
collection of DDPG makes: ``get_actions(t, observations, policy)`` on device tensors, one row per env."""


class ExplorationStrategy(object):
    def get_action(self, t, observation, policy, **kwargs):
        raise NotImplementedError

    def get_actions(self, t, observations, policy, **kwargs):
        raise NotImplementedError

    def reset(self, mask=None):
        pass
