"""DeterministicMLPPolicy (API of rllab/policies/deterministic_mlp_policy.py:12-73): action = MLP(observation), the actor
of DDPG.

The reference builds it with Lasagne: rectify hidden layers with He-uniform weights (bound sqrt(6 / fan_in)) and zero
biases, a tanh output layer whose weights AND biases are uniform in +-3e-3.  Here the parameters live in ONE flat float32
device vector in the reference's flat order W0,b0,W1,b1,Wout,bout with W stored [in, out] row-major, as every other
policy's do.  The update of DDPG runs in rl_ddpg_update (algos/ddpg_update.py); this module is the torch face: acting
(``get_action`` / ``get_actions``), snapshots, and the forward pass the tests restate the update on.
"""
import numpy as np
import torch

from rllab_amd.core.network import MLP, rectify, tanh
from rllab_amd.core.serializable import Serializable
from rllab_amd.policies.base import Policy
from rllab_amd.policies.gaussian_mlp_policy import _default_device

OUTPUT_INIT = 3e-3          # Uniform(-3e-3, 3e-3) of the output layer's W and b


def init_ddpg_mlp(net, flat):
    """The reference's initialisation of a DDPG network into the numpy vector ``flat`` (np.random): hidden W
    He-uniform (lasagne.init.HeUniform: bound sqrt(6 / fan_in)), hidden b zero, output W and b Uniform(-3e-3, 3e-3)."""
    n_layers = len(net.params) // 2
    for li in range(n_layers):
        w, b = net.params[2 * li], net.params[2 * li + 1]
        if li < n_layers - 1:
            bound = np.sqrt(6.0 / w.shape[0])
            flat[w.offset:w.offset + w.size] = np.random.uniform(-bound, bound, size=w.shape).reshape(-1)
            flat[b.offset:b.offset + b.size] = 0.0
        else:
            flat[w.offset:w.offset + w.size] = np.random.uniform(-OUTPUT_INIT, OUTPUT_INIT, size=w.shape).reshape(-1)
            flat[b.offset:b.offset + b.size] = np.random.uniform(-OUTPUT_INIT, OUTPUT_INIT, size=b.shape)


class DeterministicMLPPolicy(Policy, Serializable):
    def __init__(self, env_spec, hidden_sizes=(32, 32), hidden_nonlinearity=rectify, output_nonlinearity=tanh, bn=False):
        Serializable.quick_init(self, locals())
        if bn:
            raise NotImplementedError("DeterministicMLPPolicy(bn=True): batch normalisation is not built into the DDPG "
                                      "update kernel")
        Policy.__init__(self, env_spec)
        self.obs_dim = env_spec.observation_space.flat_dim
        self.action_dim = env_spec.action_space.flat_dim
        self.hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.hidden_nonlinearity = hidden_nonlinearity
        self.output_nonlinearity = output_nonlinearity
        self._network = MLP((self.obs_dim,), self.action_dim, self.hidden_sizes, hidden_nonlinearity,
                            output_nonlinearity, offset=0)
        self._params = list(self._network.params)
        for p in self._params:
            p._owner = self
        flat = np.zeros(self._network.end_offset, dtype=np.float32)
        init_ddpg_mlp(self._network, flat)
        self.flat_params = torch.tensor(flat, dtype=torch.float32, device=_default_device())

    # -- Parameterized ------------------------------------------------------------------------------------------------
    def get_params_internal(self, **tags):
        return [p for p in self._params if all(p.tags.get(k, False) == v for k, v in tags.items())]

    @property
    def vectorized(self):
        return True

    # -- forward ------------------------------------------------------------------------------------------------------
    def action_planes(self, obs_planes, flat=None):
        """obs [Do, B] -> actions [Da, B]."""
        flat = self.flat_params if flat is None else flat
        return self._network.forward_planes(obs_planes.to(flat.dtype), flat)

    def get_action_sym(self, obs_var, flat=None):
        """[B, Do] tensor -> [B, Da] tensor (differentiable in ``flat``)."""
        flat = self.flat_params if flat is None else flat
        obs_var = torch.as_tensor(obs_var, dtype=flat.dtype, device=flat.device)
        return self.action_planes(obs_var.t(), flat).t()

    def get_action(self, observation):
        flat_obs = self.observation_space.flatten(observation)
        with torch.no_grad():
            action = self.get_action_sym(np.asarray(flat_obs)[None, :])[0]
        return action.cpu().numpy().astype(np.float64), dict()

    def get_actions(self, observations):
        """Tensor in ([n, Do], on the env's device) -> tensor out, as the vectorised samplers call it; anything else is
        flattened like the reference does and comes back as numpy.  ``mean`` is what the sampler's per-transition loop
        records as agent_info: the action itself."""
        if torch.is_tensor(observations):
            with torch.no_grad():
                actions = self.get_action_sym(observations)
            return actions, dict(mean=actions)
        flat_obs = self.observation_space.flatten_n(observations)
        with torch.no_grad():
            actions = self.get_action_sym(np.asarray(flat_obs)).cpu().numpy().astype(np.float64)
        return actions, dict()

    def recorded_log_std(self):
        """What the sampler's per-transition loop stores as the batch's one log_std row: a deterministic policy has no
        spread, log(0)."""
        return torch.full((self.action_dim,), float("-inf"), dtype=torch.float32, device=self.flat_params.device)

    # -- the fused rollout (rl_rollout_deterministic_mlp) ----------------------------------------------------------------
    def why_no_rollout_layout(self):
        """One sentence naming what keeps this network off rl_rollout_deterministic_mlp, or None: the kernel runs the
        shapes the DDPG update kernel runs."""
        from rllab_amd import _lib
        from rllab_amd.algos.ddpg_update import MAX_ACT, MAX_HIDDEN, MAX_OBS, _activation_code
        hs = self.hidden_sizes
        if len(hs) != 2 or not all(1 <= h <= MAX_HIDDEN for h in hs):
            return "hidden_sizes=%r: the deterministic rollout kernel runs two hidden layers of 1 .. %d units" % (
                tuple(hs), MAX_HIDDEN)
        if self.obs_dim > MAX_OBS or self.action_dim > MAX_ACT:
            return "obs_dim %d, act_dim %d: the deterministic rollout kernel runs at most %d observation and %d action " \
                   "entries" % (self.obs_dim, self.action_dim, MAX_OBS, MAX_ACT)
        hidden, why = _activation_code(self.hidden_nonlinearity, "the hidden_nonlinearity", "rectify or tanh")
        if why is None and hidden == _lib.ACT_IDENTITY:
            why = "the hidden_nonlinearity is the identity: the deterministic rollout kernel evaluates rectify or tanh"
        if why is not None:
            return why
        out, why = _activation_code(self.output_nonlinearity, "the output_nonlinearity", "tanh or the identity")
        if why is None and out == _lib.ACT_RECTIFY:
            why = "the output_nonlinearity is rectify: the deterministic rollout kernel evaluates tanh or the identity"
        return why

    def rollout_layout(self):
        """``(theta, (H0p, H1p), (hidden code, output code))`` for rl_rollout_deterministic_mlp: the parameters as one
        flat float32 vector W0[D][H0p] b0 W1[H0p][H1p] b1 W2[H1p][A] b2 on the device of ``flat_params``, each hidden
        width padded to a multiple of 4 with zero weights and biases (a padded unit is act(0) = 0 and feeds zero rows:
        exact).  Built from ``flat_params`` as they are now by one scatter on the device: no host synchronisation."""
        from rllab_amd.algos.ddpg_update import _activation_code, _net_index
        why = self.why_no_rollout_layout()
        if why is not None:
            raise NotImplementedError("DeterministicMLPPolicy: %s" % why)
        h0, h1 = self.hidden_sizes
        H0, H1 = (h0 + 3) // 4 * 4, (h1 + 3) // 4 * 4
        flat = self.flat_params
        cached = self.__dict__.get("_rollout_index")
        if cached is None or cached[0].device != flat.device:
            idx, total = _net_index(self.obs_dim, h0, h1, H0, H1, 0, self.action_dim, 0)
            cached = self._rollout_index = (torch.as_tensor(idx, device=flat.device), int(total))
        theta = torch.zeros(cached[1], dtype=torch.float32, device=flat.device)
        theta[cached[0]] = flat.detach().to(torch.float32)
        codes = (_activation_code(self.hidden_nonlinearity, "", "")[0], _activation_code(self.output_nonlinearity, "", "")[0])
        return theta, (H0, H1), codes

    def why_no_kernel_layout(self):
        """The sentence the sampler logs for a policy it steps one transition at a time."""
        return "DeterministicMLPPolicy has no rollout kernel (a fused DDPG collection rollout is not built)"
