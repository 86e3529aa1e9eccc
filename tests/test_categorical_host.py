"""Discrete actions on the host: Discrete, Categorical, GridWorldEnv, CategoricalMLPPolicy and categorical batches
(no GPU).  The reference's own files are rllab/spaces/discrete.py, rllab/distributions/categorical.py,
rllab/envs/grid_world_env.py and rllab/policies/categorical_mlp_policy.py."""
import pickle

import numpy as np
import pytest
import torch

MAP_TEXT = {
    "chain": ["GFFFFFFFFFFFFFSFFFFFFFFFFFFFG"],
    "4x4_safe": ["SFFF", "FWFW", "FFFW", "WFFG"],
    "4x4": ["SFFF", "FHFH", "FFFH", "HFFG"],
}


# -- Discrete -----------------------------------------------------------------------------------------------------------
def test_discrete_flatten_round_trips():
    from rllab.spaces import Discrete
    sp = Discrete(5)
    assert sp.flat_dim == 5 and sp.n == 5
    for i in range(5):
        one_hot = sp.flatten(i)
        assert one_hot.shape == (5,) and one_hot.sum() == 1 and one_hot[i] == 1
        assert sp.unflatten(one_hot) == i
    idx = np.array([4, 0, 2, 2, 1])
    flat = sp.flatten_n(idx)
    assert flat.shape == (5, 5) and np.array_equal(flat.argmax(axis=1), idx) and np.all(flat.sum(axis=1) == 1)
    assert np.array_equal(sp.unflatten_n(flat), idx)
    assert sp.contains(3) and sp.contains(np.int64(0)) and not sp.contains(5) and not sp.contains(-1)
    assert not sp.contains(1.0) and not sp.contains(np.array([1]))
    np.random.seed(0)
    assert all(sp.contains(sp.sample()) for _ in range(20))
    assert sp == Discrete(5) and sp != Discrete(4) and hash(sp) == hash(Discrete(5))


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_discrete_weighted_sample_follows_the_cumulative_rule(seed):
    """idx = sum(cumsum(weights) < u), then min(idx, n - 1)  (rllab/misc/special.py:10-19)."""
    from rllab.spaces import Discrete
    sp = Discrete(4)
    rng = np.random.RandomState(100 + seed)
    for _ in range(25):
        w = rng.dirichlet(np.ones(4))
        np.random.seed(seed)
        got = sp.weighted_sample(w)
        np.random.seed(seed)
        u = np.random.rand()
        want = min(int(np.sum(np.cumsum(w) < u)), 3)
        assert got == want
    # cumulative sums that stop short of u: clamped to the last index
    np.random.seed(3)
    assert sp.weighted_sample(np.zeros(4)) == 3


# -- Categorical --------------------------------------------------------------------------------------------------------
def _random_probs(rng, n, a):
    return rng.dirichlet(np.ones(a), size=n)


def test_categorical_numpy_and_torch_twins_agree():
    from rllab.distributions.categorical import Categorical
    rng = np.random.RandomState(0)
    dist = Categorical(4)
    assert dist.dim == 4 and dist.dist_info_keys == ["prob"]
    p, q = _random_probs(rng, 50, 4), _random_probs(rng, 50, 4)
    x = np.eye(4)[rng.randint(0, 4, size=50)]
    tp, tq, tx = torch.as_tensor(p), torch.as_tensor(q), torch.as_tensor(x)
    assert np.abs(dist.kl(dict(prob=p), dict(prob=q)) - dist.kl_sym(dict(prob=tp), dict(prob=tq)).numpy()).max() < 1e-12
    assert np.abs(dist.entropy(dict(prob=p)) - dist.entropy_sym(dict(prob=tp)).numpy()).max() < 1e-12
    assert np.abs(dist.log_likelihood(x, dict(prob=p)) - dist.log_likelihood_sym(tx, dict(prob=tp)).numpy()).max() < 1e-12
    lr = dist.likelihood_ratio_sym(tx, dict(prob=tp), dict(prob=tq)).numpy()
    assert np.abs(lr - (np.sum(q * x, -1) + 1e-8) / (np.sum(p * x, -1) + 1e-8)).max() < 1e-12
    # the engine's planes: the action axis first
    P, Q, X = dict(prob=tp.t()), dict(prob=tq.t()), tx.t()
    assert torch.equal(dist.kl_sym(P, Q, axis=0), dist.kl_sym(dict(prob=tp), dict(prob=tq)))
    assert torch.equal(dist.entropy_sym(P, axis=0), dist.entropy_sym(dict(prob=tp)))
    assert torch.equal(dist.log_likelihood_sym(X, P, axis=0), dist.log_likelihood_sym(tx, dict(prob=tp)))
    assert torch.equal(dist.likelihood_ratio_sym(X, P, Q, axis=0), dist.likelihood_ratio_sym(tx, dict(prob=tp), dict(prob=tq)))


def test_categorical_identities():
    from rllab.distributions.categorical import TINY, Categorical
    assert TINY == 1e-8
    dist = Categorical(4)
    p = _random_probs(np.random.RandomState(1), 20, 4)
    assert np.all(dist.kl(dict(prob=p), dict(prob=p)) == 0)
    uniform = np.full((1, 4), 0.25)
    assert dist.entropy(dict(prob=uniform))[0] == pytest.approx(-np.log(0.25 + 1e-8), abs=1e-15)
    x = np.eye(4)[[0, 3, 1, 2] * 5]
    lr = dist.likelihood_ratio_sym(torch.as_tensor(x), dict(prob=torch.as_tensor(p)), dict(prob=torch.as_tensor(p)))
    assert torch.all(lr == 1)
    assert np.all(dist.likelihood_ratio(x, dict(prob=p), dict(prob=p)) == 1)


# -- GridWorldEnv -------------------------------------------------------------------------------------------------------
def _table_from_text(rows):
    """(next_state, reward, done) for every (state, action), derived from the map text alone."""
    n_row, n_col = len(rows), len(rows[0])
    moves = {0: (0, -1), 1: (1, 0), 2: (0, 1), 3: (-1, 0)}      # left, down, right, up
    table = {}
    for r in range(n_row):
        for c in range(n_col):
            for a, (dr, dc) in moves.items():
                r2, c2 = min(max(r + dr, 0), n_row - 1), min(max(c + dc, 0), n_col - 1)
                if rows[r2][c2] == "W" or rows[r][c] in "HG":
                    r2, c2 = r, c
                cell = rows[r2][c2]
                table[(r * n_col + c, a)] = (r2 * n_col + c2, 1 if cell == "G" else 0, cell in "HG")
    return table


@pytest.mark.parametrize("name", ["4x4", "4x4_safe", "chain"])
def test_gridworld_transitions_match_the_map(name):
    from rllab.envs.grid_world_env import GridWorldEnv
    from rllab.spaces import Discrete
    rows = MAP_TEXT[name]
    env = GridWorldEnv(name)
    n_states = len(rows) * len(rows[0])
    assert env.observation_space == Discrete(n_states) and env.action_space == Discrete(4)
    assert env.reset() == "".join(rows).index("S") == env.start_state
    table = _table_from_text(rows)
    seen = dict(border=0, wall=0, hole=0, goal=0)
    for (s, a), (s2, rew, done) in sorted(table.items()):
        if "".join(rows)[s] == "W":
            continue                                  # nobody ever stands inside a wall
        assert env.get_possible_next_states(s, a) == [(s2, 1.0)]
        env.state = s
        if "".join(rows)[s] in "HG":
            continue                                  # (an episode ends there: the next step is a reset)
        obs, reward, d, info = env.step(a)
        assert (obs, reward, d) == (s2, rew, done) and env.state == s2 and isinstance(obs, (int, np.integer))
        cell = "".join(rows)[s2]
        seen["hole"] += cell == "H" and rew == 0 and done
        seen["goal"] += cell == "G" and rew == 1 and done
        seen["border"] += s2 == s and cell not in "HG"
    assert seen["border"] > 0 and seen["goal"] > 0
    if name == "4x4":
        assert seen["hole"] > 0
    if name == "4x4_safe":
        # the wall at (1, 1) blocks a step down from (0, 1), right from (1, 0), up from (2, 1)
        assert table[(1, 1)][0] == 1 and table[(4, 2)][0] == 4 and table[(9, 3)][0] == 9


def test_gridworld_aliases_maps_and_directions():
    from rllab.envs.grid_world_env import GridWorldEnv
    a = GridWorldEnv(["S.x", "o.G"])
    b = GridWorldEnv(["SFW", "HFG"])
    assert np.array_equal(a.desc, b.desc) and a.start_state == 0 and (a.n_row, a.n_col) == (2, 3)
    assert list(a.cell_codes()) == [0, 0, 1, 2, 0, 3]
    assert [GridWorldEnv.action_from_direction(d) for d in ("left", "down", "right", "up")] == [0, 1, 2, 3]
    assert GridWorldEnv("8x8").observation_space.n == 64 and GridWorldEnv().observation_space.n == 16
    assert GridWorldEnv().vectorized


# -- CategoricalMLPPolicy ----------------------------------------------------------------------------------------------
def _policy(hidden=(32, 32), desc="4x4", seed=0):
    from rllab.envs.grid_world_env import GridWorldEnv
    from rllab.policies.categorical_mlp_policy import CategoricalMLPPolicy
    np.random.seed(seed)
    env = GridWorldEnv(desc)
    return env, CategoricalMLPPolicy(env_spec=env.spec, hidden_sizes=hidden)


def test_policy_flat_parameter_order_is_the_mean_networks():
    env, pol = _policy((8, 6))
    shapes = [(16, 8), (8,), (8, 6), (6,), (6, 4), (4,)]
    assert pol.get_param_shapes() == shapes
    assert [p.name for p in pol.get_params()] == ["hidden_0.W", "hidden_0.b", "hidden_1.W", "hidden_1.b", "output.W",
                                                  "output.b"]
    theta = np.random.RandomState(5).randn(sum(int(np.prod(s)) for s in shapes)) * 0.3
    pol.set_param_values(theta)
    assert np.allclose(pol.get_param_values(), theta, atol=1e-7)
    W0, b0, W1, b1, Wo, bo = pol.flat_to_params(theta.astype(np.float32).astype(np.float64))
    obs = np.eye(16)[[0, 5, 15]]
    logits = np.tanh(np.tanh(obs @ W0 + b0) @ W1 + b1) @ Wo + bo
    want = np.exp(logits - logits.max(axis=1, keepdims=True))
    want /= want.sum(axis=1, keepdims=True)
    got = pol.dist_info(obs)["prob"]
    assert got.shape == (3, 4) and np.abs(got - want).max() < 1e-6
    planes = pol.dist_info_planes(torch.as_tensor(obs.T, dtype=torch.float32, device=pol.flat_params.device))["prob"]
    assert planes.shape == (4, 3) and np.abs(planes.cpu().numpy().T - want).max() < 1e-6
    # the same order as GaussianMLPPolicy's mean network
    from rllab.envs.env_spec import EnvSpec
    from rllab.policies.gaussian_mlp_policy import GaussianMLPPolicy
    from rllab.spaces import Box
    g = GaussianMLPPolicy(EnvSpec(Box(-1, 1, (16,)), Box(-1, 1, (4,))), hidden_sizes=(8, 6))
    assert g.get_param_shapes()[:6] == shapes


def test_policy_actions_and_pickle_round_trip():
    env, pol = _policy((20,))
    obs = env.reset()
    np.random.seed(11)
    action, info = pol.get_action(obs)
    assert env.action_space.contains(action) and info["prob"].shape == (4,) and abs(info["prob"].sum() - 1) < 1e-6
    np.random.seed(11)
    u = np.random.rand()
    assert action == min(int(np.sum(np.cumsum(info["prob"]) < u)), 3)
    assert pol.get_action(obs, deterministic=True)[0] == int(np.argmax(info["prob"]))
    actions, infos = pol.get_actions([0, 3, 7])
    assert len(actions) == 3 and infos["prob"].shape == (3, 4)
    assert pol.distribution.dist_info_keys == ["prob"] and not pol.recurrent and pol.vectorized
    v0 = pol.param_version()
    pol.set_param_values(pol.get_param_values() * 1.5)
    assert pol.param_version() != v0
    twin = pickle.loads(pickle.dumps(pol))
    assert twin.hidden_sizes == (20,) and np.array_equal(twin.get_param_values(), pol.get_param_values())
    assert np.array_equal(twin.dist_info(np.eye(16))["prob"], pol.dist_info(np.eye(16))["prob"])
    env2 = pickle.loads(pickle.dumps(type(env)(["S.x", "o.G"])))
    assert (env2.n_row, env2.n_col) == (2, 3) and list(env2.cell_codes()) == [0, 0, 1, 2, 0, 3]


def test_policy_says_why_it_leaves_the_kernels():
    env, pol = _policy((32, 32), "8x8")
    assert pol.fused_ops() is None and "64" in pol.why_no_kernel_layout()
    from rllab.policies.categorical_mlp_policy import CategoricalMLPPolicy
    seq = CategoricalMLPPolicy(env_spec=env.spec, num_seq_inputs=2)
    assert seq.obs_dim == 128 and "num_seq_inputs" in seq.why_no_kernel_layout()


# -- categorical batches ------------------------------------------------------------------------------------------------
def test_pathlist_of_a_categorical_batch():
    from rllab.sampler.trajectories import PathList, Trajectories
    T, N, S, A = 5, 2, 3, 4
    rng = np.random.RandomState(2)
    states, acts = rng.randint(0, S, size=(T, N)), rng.randint(0, A, size=(T, N))
    obs = torch.as_tensor(np.eye(S)[states].transpose(2, 0, 1).copy(), dtype=torch.float32)
    act = torch.as_tensor(np.eye(A)[acts].transpose(2, 0, 1).copy(), dtype=torch.float32)
    prob = torch.as_tensor(rng.dirichlet(np.ones(A), size=(T, N)).transpose(2, 0, 1).copy(), dtype=torch.float32)
    rew = torch.as_tensor(rng.rand(T, N), dtype=torch.float32)
    dones = torch.zeros((T, N), dtype=torch.uint8)
    dones[1, 0] = dones[4, 0] = dones[4, 1] = 1
    traj = Trajectories(obs, act, prob, None, rew, dones, T, categorical=True)
    assert traj.categorical and traj.log_std is None and (traj.obs_dim, traj.act_dim) == (S, A)
    paths = PathList(traj)
    assert len(paths) == 3
    lens = [len(p["rewards"]) for p in paths]
    assert lens == [2, 3, 5]
    p = paths[1]                                               # env 0, steps 2 .. 4
    assert set(p["agent_infos"]) == {"prob"} and p["agent_infos"]["prob"].shape == (3, A)
    assert np.array_equal(p["observations"], np.eye(S)[states[2:5, 0]]) and np.array_equal(p["actions"], np.eye(A)[acts[2:5, 0]])
    assert np.allclose(p["agent_infos"]["prob"], prob[:, 2:5, 0].t().numpy())
    both = Trajectories.concat([traj, traj])
    assert both.categorical and both.T == 2 * T and both.first_steps(3).categorical
    from rllab.sampler.base import SamplesData
    traj.valid = torch.ones((T, N), dtype=torch.bool)
    infos = SamplesData(_traj=traj)["agent_infos"]
    assert set(infos) == {"prob"} and infos["prob"].shape == (T * N, A)
