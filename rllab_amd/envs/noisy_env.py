"""NoisyObservationEnv and DelayedActionEnv (API of rllab/envs/noisy_env.py): two of the three task modifiers that make a
task partially observable -- noisy sensors, delayed actions; the third, limited sensors, is envs/occlusion_env.py.

Each stands in front of a HIP-native continuous env or in front of another of the three (at most one of each kind);
``normalize(...)`` may sit outside.  The single-env face (``reset`` / ``step`` / ``get_current_obs``) is numpy around the
wrapped env.  On the vectorised path nothing is wrapped: ``vec_env_executor`` asks the wrapped env for its ``HipVecEnv``
and sets one option on it --

    NoisyObservationEnv   ``rl_env_cfg.obs_noise``: the env kernels add obs_noise * N(0,1) to every entry of the observation
                          they produce, at a reset and at a step, from the in-kernel Philox stream (or injected draws)
    DelayedActionEnv      ``HipVecEnv.action_delay``: the executor's queue of ``action_delay`` actions per env; inside the
                          fused recurrent rollout the queue is an LDS ring (csrc/gru_kernels.hip)
    OcclusionEnv          the executor's row filter: callers see the kept rows of the full observation

The kernels always draw the noise for the FULL observation and the rows are dropped afterwards.  The draws are independent
per entry, so the kept rows carry obs_noise * N(0,1) each whichever of OcclusionEnv / NoisyObservationEnv is the outer one:
the reference's distribution under either nesting order.
"""
import numpy as np

from rllab_amd.core.serializable import Serializable
from rllab_amd.envs.base import Step
from rllab_amd.envs.proxy_env import ProxyEnv


def base_env_of(wrapper, env):
    """The HIP-native continuous env at the bottom of ``env``, which ``wrapper`` is about to stand in front of; raises
    with a sentence when the chain below is not task modifiers (one of each kind at most) over such an env."""
    from rllab_amd.envs.hip_env import HipEnv
    from rllab_amd.envs.occlusion_env import OcclusionEnv
    modifiers = (OcclusionEnv, NoisyObservationEnv, DelayedActionEnv)
    seen = [type(wrapper)]
    while isinstance(env, modifiers):
        if type(env) in seen:
            raise ValueError("%s: there is already a %s below (use at most one of each kind)" % (
                type(wrapper).__name__, type(env).__name__))
        seen.append(type(env))
        env = env.wrapped_env
    if not isinstance(env, HipEnv):
        raise NotImplementedError(
            "%s over %s: the task modifiers set options of the HIP env kernels, so they stand in front of a HIP-native "
            "continuous env (or another of OcclusionEnv / NoisyObservationEnv / DelayedActionEnv); GridWorldEnv's discrete "
            "observation has no rows to drop or to add noise to, and its rollout kernels carry no action queue" % (
                type(wrapper).__name__, type(env).__name__))
    return env


class _TaskModifier(ProxyEnv, Serializable):
    """What the three modifiers share: the check of what they wrap and the vectorised boundary."""

    def _wrap(self, env):
        self._base_env = base_env_of(self, env)
        ProxyEnv.__init__(self, env)

    @property
    def vectorized(self):
        return True

    def _configure(self, vec_env):
        raise NotImplementedError

    def vec_env_executor(self, *args, **kwargs):
        """The wrapped env's ``HipVecEnv`` with this modifier's option set on it."""
        return self._configure(self._wrapped_env.vec_env_executor(*args, **kwargs))


class NoisyObservationEnv(_TaskModifier):
    """observation + obs_noise * N(0,1), entry-wise, at ``reset`` and at ``step`` (this makes the task non-Markovian)."""

    def __init__(self, env, obs_noise=1e-1):
        Serializable.quick_init(self, locals())
        if obs_noise < 0:
            raise ValueError("obs_noise must be >= 0, got %r" % (obs_noise,))
        self._wrap(env)
        if float(self._base_env._cfg.get("obs_noise", 0.0)) != 0.0:
            raise ValueError("NoisyObservationEnv over %s(obs_noise=%g): the env kernels take one obs_noise "
                             "(rl_env_cfg.obs_noise) and one draw per entry, which cannot carry the two independent draws "
                             "of the env's own noise and this wrapper's; give the env obs_noise=0 or drop the wrapper" % (
                                 type(self._base_env).__name__, float(self._base_env._cfg["obs_noise"])))
        self.obs_noise = float(obs_noise)

    def get_obs_noise_scale_factor(self, obs):
        return np.ones_like(obs)

    def inject_obs_noise(self, obs):
        obs = np.asarray(obs, dtype=np.float64)
        return obs + self.get_obs_noise_scale_factor(obs) * self.obs_noise * np.random.normal(size=obs.shape)

    def get_current_obs(self):
        return self.inject_obs_noise(self._wrapped_env.get_current_obs())

    def reset(self):
        return self.inject_obs_noise(self._wrapped_env.reset())

    def step(self, action):
        next_obs, reward, done, info = self._wrapped_env.step(action)
        return Step(self.inject_obs_noise(next_obs), reward, done, **info)

    def _configure(self, vec_env):
        return vec_env.override_cfg(obs_noise=self.obs_noise)


class DelayedActionEnv(_TaskModifier):
    """The env is stepped with the action it was handed ``action_delay`` steps ago; the first ``action_delay`` steps of a
    path apply zeros."""

    def __init__(self, env, action_delay=3):
        Serializable.quick_init(self, locals())
        if int(action_delay) != action_delay or action_delay < 1:
            raise ValueError("action_delay must be an integer >= 1, got %r (a delay of 0 is the env itself)" % (
                action_delay,))
        self._wrap(env)
        self.action_delay = int(action_delay)
        self._queued_actions = None

    def reset(self):
        obs = self._wrapped_env.reset()
        self._queued_actions = np.zeros((self.action_delay, self.action_dim))
        return obs

    def step(self, action):
        if self._queued_actions is None:
            raise RuntimeError("DelayedActionEnv.step before reset: the action queue starts at a reset")
        action = np.asarray(action, dtype=np.float64).reshape(self.action_dim)
        next_obs, reward, done, info = self._wrapped_env.step(self._queued_actions[0])
        self._queued_actions = np.concatenate([self._queued_actions[1:], action[None]])
        return Step(next_obs, reward, done, **info)

    def _configure(self, vec_env):
        return vec_env.delay_actions(self.action_delay)
