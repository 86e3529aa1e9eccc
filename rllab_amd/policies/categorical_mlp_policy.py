"""CategoricalMLPPolicy (API of rllab/policies/categorical_mlp_policy.py:15-85).

prob = softmax(MLP(tanh hidden layers, linear output)) over a ``Discrete`` action space.  The reference builds this with
Lasagne (``MLP(output_nonlinearity=softmax)``, rllab/core/network.py:36-101); here the parameters live in ONE flat
float32 device vector in the reference's flat order W0,b0,W1,b1,...,Wout,bout with W stored [in, out] row-major --
the order of ``GaussianMLPPolicy``'s mean network -- Glorot-uniform weights and zero biases.

On a ``Discrete`` observation space observations are one-hot, so the policy is a function of the state index alone:
``prob_table()`` is that function as a table ``[n_actions, n_states]``, what the fused GridWorld rollout samples from.
"""
import numpy as np
import torch

from rllab_amd.core.network import MLP, tanh
from rllab_amd.core.serializable import Serializable
from rllab_amd.distributions.categorical import Categorical
from rllab_amd.policies.base import StochasticPolicy
from rllab_amd.policies.gaussian_mlp_policy import _default_device
from rllab_amd.spaces import Discrete


def softmax(x):
    """Softmax over the action axis of logit PLANES [A, B] (the engine's layout: feature axis first)."""
    return torch.softmax(x, dim=0)


class CategoricalMLPPolicy(StochasticPolicy, Serializable):
    def __init__(self, env_spec, hidden_sizes=(32, 32), hidden_nonlinearity=tanh, num_seq_inputs=1, prob_network=None):
        """``prob_network``: an MLP description (core/network.py) whose layer sizes and hidden nonlinearity are taken
        over -- its parameters are re-created in this policy's flat vector; the output is a softmax either way."""
        Serializable.quick_init(self, locals())
        assert isinstance(env_spec.action_space, Discrete)
        StochasticPolicy.__init__(self, env_spec)
        self.num_seq_inputs = int(num_seq_inputs)
        self.obs_dim = env_spec.observation_space.flat_dim * self.num_seq_inputs
        self.action_dim = env_spec.action_space.n
        if prob_network is not None:
            assert prob_network.input_dim == self.obs_dim and prob_network.output_dim == self.action_dim
            hidden_sizes, hidden_nonlinearity = prob_network.hidden_sizes, prob_network.hidden_nonlinearity
        self.hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.hidden_nonlinearity = hidden_nonlinearity
        # the logit network; the softmax is applied on top (dist_info_planes), so that the kernels' head can start from
        # the logits
        self._logit_network = MLP((self.obs_dim,), self.action_dim, self.hidden_sizes, hidden_nonlinearity, None, offset=0)
        self._params = list(self._logit_network.params)
        for p in self._params:
            p._owner = self
        self._dist = Categorical(self.action_dim)
        flat = np.zeros(self._logit_network.end_offset, dtype=np.float32)
        self._logit_network.init_values(flat)        # np.random: CPU oracle and GPU share theta under a seed
        self.flat_params = torch.tensor(flat, dtype=torch.float32, device=_default_device())

    # -- Parameterized ----------------------------------------------------------------------------------------------
    def get_params_internal(self, **tags):
        return [p for p in self._params if all(p.tags.get(k, False) == v for k, v in tags.items())]

    @property
    def vectorized(self):
        return True

    @property
    def distribution(self):
        return self._dist

    def param_version(self):
        """Changes whenever the parameters do: torch's in-place version counter plus the writes the kernels make through
        raw pointers (rl_line_search_point, rl_adam_step), which torch cannot see."""
        return (self.flat_params._version, getattr(self, "_raw_writes", 0))

    def note_raw_write(self):
        self._raw_writes = getattr(self, "_raw_writes", 0) + 1

    # -- forward ------------------------------------------------------------------------------------------------------
    def logit_planes(self, obs_planes, flat=None):
        """obs [Do, B] -> logits [A, B]."""
        flat = self.flat_params if flat is None else flat
        return self._logit_network.forward_planes(obs_planes.to(flat.dtype), flat)

    def dist_info_planes(self, obs_planes, flat=None):
        """obs [Do, B] -> dict(prob [A, B]): the sample axis last."""
        return dict(prob=softmax(self.logit_planes(obs_planes, flat)))

    def dist_info_sym(self, obs_var, state_info_vars=None):
        """[B, Do] tensor -> dict(prob [B, A])."""
        obs_var = torch.as_tensor(obs_var, dtype=self.flat_params.dtype, device=self.flat_params.device)
        return dict(prob=self.dist_info_planes(obs_var.t())["prob"].t())

    def dist_info(self, obs, state_infos=None):
        with torch.no_grad():
            d = self.dist_info_sym(np.asarray(obs))
        return {k: v.cpu().numpy().astype(np.float64) for k, v in d.items()}

    def get_action(self, observation, deterministic=False):
        flat_obs = self.observation_space.flatten(observation)
        prob = self.dist_info(flat_obs[None, :])["prob"][0]
        if deterministic:
            action = int(np.argmax(prob))
        else:
            action = self.action_space.weighted_sample(prob)
        return action, dict(prob=prob)

    def get_actions(self, observations):
        flat_obs = self.observation_space.flatten_n(observations)
        probs = self.dist_info(flat_obs)["prob"]
        actions = list(map(self.action_space.weighted_sample, probs))
        return actions, dict(prob=probs)

    # -- what the HIP kernels read ----------------------------------------------------------------------------------
    def why_no_kernel_layout(self):
        """One sentence naming what keeps this policy's update off the HIP kernels, or None."""
        if self.num_seq_inputs != 1:
            return "num_seq_inputs = %d: the kernels take one observation per sample" % self.num_seq_inputs
        from rllab_amd.policies.planes_ops import KernelNet
        return KernelNet.why_not(self, self._logit_network)

    def kernel_net(self):
        """The kernels' copy of the logit network (policies/planes_ops.py::KernelNet), or None."""
        if not hasattr(self, "_kernel_net"):
            from rllab_amd.policies.planes_ops import KernelNet
            self._kernel_net = KernelNet(self, self._logit_network) if self.why_no_kernel_layout() is None else None
        return self._kernel_net

    def fused_ops(self):
        """HIP-kernel loss / gradient / Fisher-vector product (policies/fused_categorical_ops.py), or None when the
        network is not one the kernels run (``why_no_kernel_layout()`` says why; torch autograd is used then)."""
        if self.kernel_net() is None:
            return None
        from rllab_amd.policies.fused_categorical_ops import FusedCategoricalOps
        return FusedCategoricalOps(self)

    def prob_table(self):
        """float32 device table ``prob[n_actions][obs_dim]``: the action probabilities at every one-hot observation, at the
        CURRENT parameters (rebuilt when they have moved).  Through the kernels (rl_mlp_forward_ws on the identity
        observation planes, rl_categorical_softmax) when the network is one they run; otherwise the policy's own torch
        forward over the one-hot rows."""
        tag = self.param_version()
        cached = getattr(self, "_table", None)
        if cached is not None and cached[0] == tag:
            return cached[1]
        net = self.kernel_net() if self.flat_params.is_cuda else None
        if net is not None:
            table = net.softmax_of_identity()
        else:
            with torch.no_grad():
                eye = torch.eye(self.obs_dim, dtype=self.flat_params.dtype, device=self.flat_params.device)
                table = self.dist_info_planes(eye)["prob"].to(torch.float32).contiguous()
        self._table = (tag, table)
        return table
