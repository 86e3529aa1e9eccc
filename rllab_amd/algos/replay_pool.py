"""DeviceReplayPool: the replay pool of DDPG (rllab/algos/ddpg.py:25-81, SimpleReplayPool) as a flat ring of ``capacity``
rows in device memory, struct-of-arrays in float32:

    obs[cap][D]  act[cap][A]  rew[cap]  term[cap]  next_obs[cap][D]  skip[cap]

Every env of a lock-step writes exactly one row per step, so ``top`` (the row the next write goes to) and ``size`` are
host integers that advance by the number of envs: nothing is read back to know them.  A write is one ``index_copy_``
per plane at the rows ``(top + i) mod capacity``.

* ``rew`` holds what the caller hands over -- DDPG stores the reward already multiplied by ``scale_reward``.
* ``term`` is 1 where the path ended, for any reason.
* ``skip`` is 1 on the rows the reference would not have added (a path cut at ``max_path_length`` while
  ``include_horizon_terminal_transitions`` is false): the row is written, because every env writes one row per step,
  and the batch draw of rl_ddpg_update passes over it.
* ``next_obs`` of a row with ``term = 1`` is not specified: the lock-step loop stores the env's own successor there, a
  launch of the fused collection rollout (``DDPG(rollout_steps=...)``) the first observation of the next path.  The
  targets y = rew + (1 - term) * discount * Q'(next_obs, ..) never read it.

Difference from the reference, on purpose: SimpleReplayPool stores no successor observation and reads row ``index + 1``
instead, which after a dropped horizon transition pairs the last kept transition of a path with the first observation
of the NEXT path, unmasked.  Here ``next_obs`` is the env's own successor observation.
"""
import torch


class DeviceReplayPool(object):
    PLANES = ("obs", "act", "rew", "term", "next_obs", "skip")

    def __init__(self, capacity, observation_dim, action_dim, device=None):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("DeviceReplayPool: capacity must be positive, got %r" % (capacity,))
        self.observation_dim, self.action_dim = int(observation_dim), int(action_dim)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
                else torch.device("cpu")
        self.device = torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs = torch.zeros((self.capacity, self.observation_dim), **f32)
        self.act = torch.zeros((self.capacity, self.action_dim), **f32)
        self.rew = torch.zeros(self.capacity, **f32)
        self.term = torch.zeros(self.capacity, **f32)
        self.next_obs = torch.zeros((self.capacity, self.observation_dim), **f32)
        self.skip = torch.zeros(self.capacity, **f32)
        self.top = 0
        self.size = 0
        self._lanes = None

    def add(self, obs, act, rew, term, next_obs, skip=None):
        """Append one row per env: ``obs`` / ``next_obs`` [n, D], ``act`` [n, A], ``rew`` / ``term`` / ``skip`` [n]
        (tensors of any float / bool dtype on the pool's device)."""
        n = int(rew.shape[0])
        if n > self.capacity:
            raise ValueError("DeviceReplayPool: %d rows in one write, the pool holds %d" % (n, self.capacity))
        if self._lanes is None or self._lanes.numel() != n:
            self._lanes = torch.arange(n, dtype=torch.int64, device=self.device)
        rows = (self._lanes + self.top) % self.capacity
        f32 = lambda x, shape: torch.as_tensor(x, device=self.device).to(torch.float32).reshape(shape)
        self.obs.index_copy_(0, rows, f32(obs, (n, self.observation_dim)))
        self.act.index_copy_(0, rows, f32(act, (n, self.action_dim)))
        self.rew.index_copy_(0, rows, f32(rew, (n,)))
        self.term.index_copy_(0, rows, f32(term, (n,)))
        self.next_obs.index_copy_(0, rows, f32(next_obs, (n, self.observation_dim)))
        self.skip.index_copy_(0, rows, torch.zeros(n, dtype=torch.float32, device=self.device) if skip is None
                              else f32(skip, (n,)))
        self.top = (self.top + n) % self.capacity
        self.size = min(self.size + n, self.capacity)

    def logical_rows(self):
        """Physical rows of the pool's contents, oldest first: ``(top - size + i) mod capacity``."""
        return (torch.arange(self.size, dtype=torch.int64, device=self.device) + (self.top - self.size)) % self.capacity
