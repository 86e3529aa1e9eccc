"""GridWorldEnv (API and transition rule of rllab/envs/grid_world_env.py:7-149) and its lock-step executor.

    'S' start    'F' or '.' free    'W' or 'x' wall    'H' or 'o' hole (ends the episode, reward 0)    'G' goal (reward 1)

Actions: 0 left, 1 down, 2 right, 3 up.  States and observations are the cell index ``row * n_col + col``; both spaces
are ``Discrete``.  ``GridWorldEnv`` is the host implementation in plain Python integers -- the oracle of the kernel.
``GridWorldVecEnv`` runs ``n`` copies on the device: observations are one-hot, so a policy is a function of the state
index alone and the whole horizon of every env is ONE launch of ``rl_rollout_gridworld`` (csrc/categorical_kernels.hip)
on the policy's probability table ``prob[n_act][n_states]``.  A ``CategoricalGRUPolicy``'s probabilities depend on each
env's hidden state: its rollout is ONE launch of ``rl_rollout_gridworld_gru`` (csrc/categorical_gru_kernels.hip), which takes
a GRU step per env and step.
"""
import ctypes

import numpy as np
import torch

from rllab_amd.core.serializable import Serializable
from rllab_amd.envs.base import Env, Step
from rllab_amd.spaces.discrete import Discrete

MAPS = {
    "chain": [
        "GFFFFFFFFFFFFFSFFFFFFFFFFFFFG"
    ],
    "4x4_safe": [
        "SFFF",
        "FWFW",
        "FFFW",
        "WFFG"
    ],
    "4x4": [
        "SFFF",
        "FHFH",
        "FFFH",
        "HFFG"
    ],
    "8x8": [
        "SFFFFFFF",
        "FFFFFFFF",
        "FFFHFFFF",
        "FFFFFHFF",
        "FFFHFFFF",
        "FHHFFFHF",
        "FHFFHFHF",
        "FFFHFFFG"
    ],
}

_ALIASES = {".": "F", "o": "H", "x": "W"}
_INCREMENTS = ((0, -1), (1, 0), (0, 1), (-1, 0))       # left, down, right, up as (d row, d col)
CELL_CODES = {"F": 0, "S": 0, "W": 1, "H": 2, "G": 3}  # the kernel's int8 map (rl_gridworld_args.cell)


class GridWorldEnv(Env, Serializable):
    def __init__(self, desc='4x4'):
        Serializable.quick_init(self, locals())
        if isinstance(desc, str):
            desc = MAPS[desc]
        rows = [[_ALIASES.get(c, c) for c in row] for row in desc]
        if not rows or any(len(r) != len(rows[0]) for r in rows) or any(c not in CELL_CODES for r in rows for c in r):
            raise ValueError("GridWorldEnv: the map is a rectangle of the letters S F W H G (or . o x)")
        self.desc = np.array(rows)
        self.n_row, self.n_col = len(rows), len(rows[0])
        starts = [r * self.n_col + c for r in range(self.n_row) for c in range(self.n_col) if rows[r][c] == 'S']
        if len(starts) != 1:
            raise ValueError("GridWorldEnv: the map has exactly one start cell 'S'")
        self.start_state = starts[0]
        self.state = None
        self.domain_fig = None

    def reset(self):
        self.state = self.start_state
        return self.state

    @staticmethod
    def action_from_direction(d):
        """The action index of a direction name (left, down, right, up)."""
        return dict(left=0, down=1, right=2, up=3)[d]

    def _cell(self, state):
        return str(self.desc[state // self.n_col][state % self.n_col])

    def step(self, action):
        action = int(action)
        possible_next_states = self.get_possible_next_states(self.state, action)
        probs = [x[1] for x in possible_next_states]
        next_state = possible_next_states[0][0] if len(probs) == 1 else \
            possible_next_states[np.random.choice(len(probs), p=probs)][0]
        kind = self._cell(next_state)
        if kind == 'H':
            done, reward = True, 0
        elif kind in ('F', 'S'):
            done, reward = False, 0
        elif kind == 'G':
            done, reward = True, 1
        else:
            raise NotImplementedError
        self.state = next_state
        return Step(observation=self.state, reward=reward, done=done)

    def get_possible_next_states(self, state, action):
        """[(s', p(s' | s, a))] with nonzero probability: the neighbouring cell, clipped at the border; a wall -- or
        standing on a hole or the goal -- leaves the state where it is."""
        state, action = int(state), int(action)
        x, y = state // self.n_col, state % self.n_col
        dx, dy = _INCREMENTS[action]
        nx = min(max(x + dx, 0), self.n_row - 1)
        ny = min(max(y + dy, 0), self.n_col - 1)
        next_state = nx * self.n_col + ny
        state_type = self._cell(state)
        if self._cell(next_state) == 'W' or state_type == 'H' or state_type == 'G':
            return [(state, 1.)]
        return [(next_state, 1.)]

    @property
    def action_space(self):
        return Discrete(4)

    @property
    def observation_space(self):
        return Discrete(self.n_row * self.n_col)

    @property
    def horizon(self):
        return None

    # -- vectorised boundary ------------------------------------------------------------------------------------------
    @property
    def vectorized(self):
        return True

    def cell_codes(self):
        """int8 [n_row * n_col]: 0 free or start, 1 wall, 2 hole, 3 goal."""
        return np.array([CELL_CODES[str(c)] for c in self.desc.reshape(-1)], dtype=np.int8)

    def vec_env_executor(self, n_envs, max_path_length, seed=None, env_offset=0, **kw):
        return GridWorldVecEnv(self, n_envs, max_path_length, seed=seed, env_offset=env_offset)


class GridWorldVecEnv(object):
    """``n`` lock-step copies of one GridWorldEnv on the current HIP device: what ``VectorizedSampler`` asks of an
    executor.  ``rollout`` is the fused kernel; ``reset`` / ``step`` (the plain VecEnv API) loop over Python envs on
    the host."""
    terminates = True          # holes and the goal end a path before max_path_length: the sampler counts finished samples
    stateful_rollouts = False
    graphable = False
    position_ids = None

    def __init__(self, env, n_envs, max_path_length, seed=None, env_offset=0):
        from rllab_amd.envs.hip_env import _fresh_seed, _require_device
        self.env = env
        self.n = int(n_envs)
        self.max_path_length = int(max_path_length) if max_path_length is not None else 0
        self.seed = _fresh_seed() if seed is None else int(seed)
        self.env_offset = int(env_offset)
        self.step_counter = 0      # global step index: RNG counter base
        self.device = _require_device()
        self.n_states = env.n_row * env.n_col
        self.cell = torch.as_tensor(env.cell_codes(), device=self.device)
        self.state = torch.full((self.n,), int(env.start_state), dtype=torch.int32, device=self.device)
        self.ts = torch.zeros((self.n,), dtype=torch.int32, device=self.device)
        self._host_envs = None

    num_envs = property(lambda self: self.n)
    action_space = property(lambda self: self.env.action_space)
    observation_space = property(lambda self: self.env.observation_space)

    @property
    def obs_rows(self):
        raise NotImplementedError("GridWorldVecEnv samples a CategoricalMLPPolicy (num_seq_inputs=1) through the fused "
                                  "rollout only: it has no per-transition device loop for other policies")

    def takes_rollout_of(self, policy):
        from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
        from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
        if isinstance(policy, CategoricalGRUPolicy):
            return (policy.obs_dim == self.n_states and policy.action_dim == 4 and policy.rollout_layout() is not None)
        return (isinstance(policy, CategoricalMLPPolicy) and policy.num_seq_inputs == 1
                and policy.obs_dim == self.n_states and policy.action_dim == 4)

    def rollout(self, policy, horizon, reset_at_start=True, u=None):
        """``horizon`` lock steps of sample -> step -> record -> auto-reset in ONE launch (rl_rollout_gridworld, or
        rl_rollout_gridworld_gru for a CategoricalGRUPolicy); returns ``Trajectories`` whose ``means`` planes hold the
        recorded action probabilities.  ``u`` [T, n]: injected uniforms (parity runs; otherwise each env's Philox
        stream).  ``reset_at_start=False``: the envs carry on from their state and step count (and, under a recurrent
        policy, from the hidden state and previous action the previous launch left on this executor)."""
        from rllab_amd import _lib
        from rllab_amd.sampler import dist as D
        from rllab_amd.sampler.trajectories import Trajectories
        if D.is_distributed():
            raise NotImplementedError("GridWorldVecEnv runs in one process on one GPU: the categorical path is not "
                                      "sharded over ranks")
        if not self.takes_rollout_of(policy):
            why = policy.why_no_rollout_kernel() if hasattr(policy, "why_no_rollout_kernel") else None
            raise NotImplementedError("the fused GridWorld rollout samples a CategoricalMLPPolicy (num_seq_inputs=1) or a "
                                      "CategoricalGRUPolicy built on this env's spec%s" % ("" if why is None else ": " + why))
        T, n, S, A = int(horizon), self.n, self.n_states, 4
        f32 = dict(dtype=torch.float32, device=self.device)
        if u is not None:
            u = torch.as_tensor(u, **f32).contiguous()
            assert u.shape == (T, n)
        obs = torch.empty((S, T, n), **f32)
        act = torch.empty((A, T, n), **f32)
        prob = torch.empty((A, T, n), **f32)
        rew = torch.empty((T, n), **f32)
        done = torch.empty((T, n), dtype=torch.uint8, device=self.device)
        env_args = dict(
            n_envs=n, horizon=T, max_path_length=self.max_path_length, reset_at_start=int(bool(reset_at_start)),
            n_row=self.env.n_row, n_col=self.env.n_col, n_act=A, start_state=int(self.env.start_state),
            env_offset=self.env_offset, seed=self.seed, step_counter=self.step_counter,
            cell=self.cell.data_ptr(), u=None if u is None else u.data_ptr(),
            state=self.state.data_ptr(), ts=self.ts.data_ptr(), obs=obs.data_ptr(), actions=act.data_ptr(),
            prob_out=prob.data_ptr(), rewards=rew.data_ptr(), dones=done.data_ptr())
        recurrent = getattr(policy, "recurrent", False)
        if recurrent:
            # the hidden state [H, n] and the previous action index [n] are buffers of this executor next to ``state`` /
            # ``ts``: written by every launch, read by one with ``reset_at_start=False``
            H = policy.kernel_hidden
            theta = policy.rollout_layout()
            assert theta.dtype == torch.float32 and theta.is_contiguous() and theta.device == self.device
            if getattr(self, "hidden_state", None) is None or tuple(self.hidden_state.shape) != (H, n):
                if not reset_at_start:
                    raise ValueError("rollout(reset_at_start=False) of a recurrent policy needs the hidden state a previous "
                                     "launch of that policy left on this executor")
                self.hidden_state = torch.zeros((H, n), **f32)
                self.prev_action = torch.full((n,), -1, dtype=torch.int32, device=self.device)
            args = _lib.GridWorldGruArgs(hidden=H, include_action=int(policy.state_include_action), theta=theta.data_ptr(),
                                         hidden_state=self.hidden_state.data_ptr(),
                                         prev_action=self.prev_action.data_ptr(), **env_args)
            _lib.check(_lib.lib.rl_rollout_gridworld_gru(ctypes.byref(args), _lib.stream_ptr()), "rl_rollout_gridworld_gru")
        else:
            table = policy.prob_table()
            assert table.shape == (A, S) and table.dtype == torch.float32 and table.is_contiguous() and table.device == self.device
            args = _lib.GridWorldArgs(prob=table.data_ptr(), **env_args)
            _lib.check(_lib.lib.rl_rollout_gridworld(ctypes.byref(args), _lib.stream_ptr()), "rl_rollout_gridworld")
        self.step_counter += T
        self._host_envs = None
        return Trajectories(obs, act, prob, None, rew, done, self.max_path_length, categorical=True,
                            prev_action_info=bool(recurrent and policy.state_include_action))

    # -- plain VecEnv API: a host loop over the Python env ------------------------------------------------------------
    def _envs(self):
        if self._host_envs is None:
            state, ts = self.state.cpu().numpy(), self.ts.cpu().numpy()
            self._host_envs = [Serializable.clone(self.env) for _ in range(self.n)]
            for e, s in zip(self._host_envs, state):
                e.state = int(s)
            self._host_ts = [int(t) for t in ts]
        return self._host_envs

    def _sync_device(self):
        self.state.copy_(torch.as_tensor([e.state for e in self._host_envs], dtype=torch.int32))
        self.ts.copy_(torch.as_tensor(self._host_ts, dtype=torch.int32))

    def reset(self):
        envs = self._envs()
        obs = [e.reset() for e in envs]
        self._host_ts = [0] * self.n
        self._sync_device()
        return obs

    def step(self, action_n):
        envs = self._envs()
        obs, rewards, dones = [], [], []
        for i, (e, a) in enumerate(zip(envs, action_n)):
            o, r, d, _ = e.step(int(np.argmax(a)) if np.ndim(a) else int(a))
            self._host_ts[i] += 1
            if self.max_path_length > 0 and self._host_ts[i] >= self.max_path_length:
                d = True
            if d:
                o = e.reset()
                self._host_ts[i] = 0
            obs.append(o)
            rewards.append(r)
            dones.append(d)
        self._sync_device()
        return obs, np.asarray(rewards, dtype=np.float64), np.asarray(dones), dict()

    def terminate(self):
        pass
