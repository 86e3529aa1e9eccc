"""Cross-entropy method (API and control flow of rllab/algos/cem.py:15-181).

Per iteration: draw candidates  x_c = cur_mean + sample_std * N(0, I)  in parameter space, score every candidate by
the return of ``n_evals`` rollouts, refit mean and std of the sampling distribution to the best ``best_frac`` of them.

The reference evaluates one candidate at a time (``_worker_rollout_policy``, :29-56: set_param_values, rollout).  Here a
whole population is ONE launch of the population rollout (``HipVecEnv.rollout_population``, rl_rollout_population; for a
GaussianGRUPolicy ``HipVecEnv.rollout_population_recurrent``, rl_rollout_population_gru -- ``population_launcher``): env
i runs candidate i % n_cand with its own parameters, and the kernel hands back, per env, discounted return,
undiscounted return and length of its first path -- everything the method needs.  Candidates are drawn, scored, sorted
and refitted on the device in float64; one host read per iteration brings the logged values.

The two functions ``cem_scores`` / ``cem_refit`` are the arithmetic of :15-27 and :137-146 on tensors of any device.
"""
import math

import numpy as np
import torch

import rllab_amd.misc.logger as logger
from rllab_amd.algos.base import RLAlgorithm
from rllab_amd.core.serializable import Serializable
from rllab_amd.misc import ext


def cem_scores(first_path, n_cand, n_evals):
    """``first_path`` [3, n_cand * n_evals] (discounted return, undiscounted return, length of env i's first path;
    env i = candidate i % n_cand, evaluation i // n_cand)  ->  (fs, undiscounted), float64 [n_cand] each: mean minus
    standard error over the candidate's evaluations (cem.py:15-27, :46-47 -- ``_get_stderr_lb_varyinglens(returns)[0]`` and
    ``_get_stderr_lb(undiscounted_returns)``: ddof 1 with several evaluations, the plain value with one)."""
    x = first_path[:2].to(torch.float64).reshape(2, int(n_evals), int(n_cand))
    mu = x.mean(dim=1)
    if int(n_evals) > 1:
        mu = mu - x.std(dim=1, unbiased=True) / math.sqrt(int(n_evals))
    return mu[0], mu[1]


def cem_refit(xs, fs, n_best):
    """(cur_mean, cur_std, best_x, best_inds) of the ``n_best`` candidates with the highest score (cem.py:142-146):
    ``best_inds = argsort(-fs)[:n_best]`` (stable: ties keep their index order), mean and std (ddof 0) of those rows of
    ``xs`` [n_cand, P], and the best row itself."""
    best_inds = torch.sort(-fs, stable=True).indices[:int(n_best)]
    best_xs = xs.index_select(0, best_inds)
    return best_xs.mean(dim=0), best_xs.std(dim=0, unbiased=False), best_xs[0], best_inds


def cem_sample_std(cur_std, extra_std, itr, extra_decay_time):
    """sqrt(cur_std^2 + extra_std^2 * max(1 - itr / extra_decay_time, 0))   (cem.py:119-120); ``cur_std`` float or tensor."""
    extra_var_mult = max(1.0 - itr / extra_decay_time, 0)
    var = cur_std ** 2 + extra_std ** 2 * extra_var_mult
    return torch.sqrt(var) if torch.is_tensor(var) else math.sqrt(var)


def cem_sample_prefix(lengths, batch_size):
    """Criterion "samples" (cem.py:50-51 under stateful_pool.run_collect): candidates count in index order, each with
    ``lengths[c]`` samples, until the count reaches ``batch_size``.  Returns the number of candidates used -- the shortest
    prefix whose lengths sum to at least ``batch_size`` -- or None while the sum of all is short (launch more)."""
    total = torch.cumsum(torch.as_tensor(lengths).to(torch.float64).reshape(-1), dim=0)
    reached = torch.nonzero(total >= float(batch_size))
    return int(reached[0]) + 1 if reached.numel() else None


def population_why_unsupported(env, policy, plot=False):
    """One sentence naming what keeps this env / policy / plot setting off the population rollout, or None (shared by the
    algorithms that evaluate candidates there: CEM, CMAES)."""
    from rllab_amd.envs.hip_env import HipEnv
    from rllab_amd.envs.normalized_env import NormalizedEnv
    from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
    from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy, is_rectify
    from rllab_amd.policies.kernel_layout import tile_for
    from rllab_amd.sampler import dist as D
    if plot:
        return "plot=True: plotting is out of scope of the engine"
    if D.is_distributed():
        return "a distributed run: the population rollout evaluates its candidates on one device"
    if isinstance(env, NormalizedEnv):
        if env._normalize_obs or env._normalize_reward:
            return ("normalize(env, normalize_obs / normalize_reward): the running estimates of a NormalizedEnv are not "
                    "part of the population rollout")
        env = env._wrapped_env
    if isinstance(getattr(env, "_base_env", None), HipEnv):
        return ("%s: the task modifiers (OcclusionEnv / NoisyObservationEnv / DelayedActionEnv) are not part of the "
                "population rollout" % type(env).__name__)
    if not isinstance(env, HipEnv):
        return "%s is not a HIP-native env (optionally wrapped in normalize)" % type(env).__name__
    if env._position_ids is not None:
        return "position_only observations: the candidates' first layers are built on the kept rows"
    if isinstance(policy, GaussianGRUPolicy):
        # the recurrent population rollout runs what the recurrent rollout runs
        return policy.why_no_rollout_kernel()
    if not isinstance(policy, GaussianMLPPolicy):
        return "%s is neither a GaussianMLPPolicy nor a GaussianGRUPolicy" % type(policy).__name__
    if policy.state_dependent_std:
        return "the log-std is a network (adaptive_std / std_network): the population kernel takes one log_std row per candidate"
    if is_rectify(policy.hidden_nonlinearity):
        return "hidden_nonlinearity is rectify: the population kernel evaluates tanh layers"
    hs = tuple(int(h) for h in policy.hidden_sizes)
    if not ((len(hs) == 1 and 1 <= hs[0] <= 64) or tile_for(hs) is not None):
        return ("hidden_sizes=%r: the population kernel runs two hidden layers of at most 64 units each, or one of at "
                "most 64" % (hs,))
    if policy.kernel_layout() is None:
        return policy.why_no_kernel_layout()
    return None


def population_launcher(policy, vec_env):
    """``launch(xs, n_evals, horizon, discount, record) -> (Trajectories or None, first_path)``: candidates ``xs`` [n_cand, P]
    (float64, the policy's parameter order) through the population rollout of this policy's family on ``vec_env`` --
    ``rollout_population`` for a GaussianMLPPolicy, ``rollout_population_recurrent`` for a GaussianGRUPolicy (shared by
    CEM and CMAES, behind ``population_why_unsupported``)."""
    log_min_std = math.log(policy.min_std) if policy.min_std is not None else None
    if getattr(policy, "recurrent", False):
        def launch(xs, n_evals, horizon, discount, record):
            return vec_env.rollout_population_recurrent(
                policy.pack_rows(xs.to(torch.float32)), n_evals, horizon, discount, policy.kernel_hidden,
                policy.state_include_action, record=record, log_min_std=log_min_std)
        return launch
    layout = policy.kernel_layout()

    def launch(xs, n_evals, horizon, discount, record):
        return vec_env.rollout_population(
            layout.pack_rows(xs.to(torch.float32)), n_evals, horizon, discount, record=record,
            layer_activations=layout.layer_activations, log_min_std=log_min_std)
    return launch


class CEM(RLAlgorithm, Serializable):
    def __init__(
            self,
            env,
            policy,
            n_itr=500,
            max_path_length=500,
            discount=0.99,
            init_std=1.,
            n_samples=100,
            batch_size=None,
            best_frac=0.05,
            extra_std=1.,
            extra_decay_time=100,
            plot=False,
            n_evals=1,
            seed=None,
            record_paths=True,
            **kwargs
    ):
        """
        :param n_itr: Number of iterations.
        :param max_path_length: Maximum length of a single rollout.
        :param batch_size: # of samples from trajs from param distribution, when this
        is set, n_samples is ignored
        :param discount: Discount.
        :param plot: Plot evaluation run after each iteration.
        :param init_std: Initial std for param distribution
        :param extra_std: Decaying std added to param distribution at each iteration
        :param extra_decay_time: Iterations that it takes to decay extra std
        :param n_samples: #of samples from param distribution
        :param best_frac: Best fraction of the sampled params
        :param n_evals: # of evals per sample from the param distr. returned score is mean - stderr of evals
        :param seed: engine option -- seed of the candidate draws and of the envs' Philox streams (None: ext.get_seed())
        :param record_paths: engine option -- False: no trajectory plane is stored (12 bytes per rollout leave the kernel)
        and env / policy log_diagnostics are skipped
        """
        Serializable.quick_init(self, locals())
        self.env = env
        self.policy = policy
        self.batch_size = batch_size
        self.plot = plot
        self.extra_decay_time = extra_decay_time
        self.extra_std = extra_std
        self.best_frac = best_frac
        self.n_samples = n_samples
        self.init_std = init_std
        self.discount = discount
        self.max_path_length = max_path_length
        self.n_itr = n_itr
        self.n_evals = n_evals
        self.seed = seed
        self.record_paths = record_paths
        # the latest iteration's population, on the device: candidates used [n, P] float64 (criterion "samples": the prefix),
        # their scores, and the counted length (last evaluation's path) of EVERY candidate launched
        self.last_n_candidates = self.last_xs = self.last_fs = self.last_lengths = None

    def why_unsupported(self):
        """One sentence naming what keeps this configuration off the population rollout, or None."""
        return population_why_unsupported(self.env, self.policy, self.plot)

    def train(self):
        reason = self.why_unsupported()
        if reason is not None:
            raise NotImplementedError("CEM: " + reason)
        policy = self.policy
        dev = policy.flat_params.device
        seed = self.seed if self.seed is not None else ext.get_seed()
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        n_evals, mpl = int(self.n_evals), int(self.max_path_length)
        # candidates of one launch: the population (criterion "paths"), or what batch_size needs if every path runs full length
        n_launch = int(self.n_samples) if self.batch_size is None else -(-int(self.batch_size) // mpl)
        vec_env = self.env.vec_env_executor(n_envs=n_launch * n_evals, max_path_length=mpl, seed=int(seed))
        launch = population_launcher(policy, vec_env)
        f64 = dict(dtype=torch.float64, device=dev)

        cur_mean = torch.as_tensor(policy.get_param_values(), **f64)
        cur_std = torch.full_like(cur_mean, float(self.init_std))
        n_best = max(1, int(self.n_samples * self.best_frac))

        for itr in range(self.n_itr):
            # sample around the current distribution
            sample_std = cem_sample_std(cur_std, self.extra_std, itr, self.extra_decay_time)
            xs_l, fp_l, traj_l, n_used = [], [], [], None
            while n_used is None:
                xs = torch.randn((n_launch, cur_mean.numel()), generator=gen, **f64) * sample_std + cur_mean
                traj, first_path = launch(xs, n_evals, mpl, self.discount, bool(self.record_paths))
                xs_l.append(xs)
                fp_l.append(first_path.view(3, n_evals, n_launch))
                traj_l.append(traj)
                if self.batch_size is None:
                    n_used = n_launch
                else:
                    # every candidate counts with the length of its LAST evaluation's path (cem.py:50-51)
                    n_used = cem_sample_prefix(torch.cat([fp[2, n_evals - 1] for fp in fp_l]), self.batch_size)
            xs = torch.cat(xs_l)[:n_used]
            first_path = torch.cat(fp_l, dim=2)[:, :, :n_used]                  # [3, n_evals, n_used]
            fs, undiscounted_returns = cem_scores(first_path.reshape(3, -1), n_used, n_evals)
            cur_mean, cur_std, best_x, _ = cem_refit(xs, fs, n_best)
            self.last_n_candidates, self.last_xs, self.last_fs = n_used, xs, fs
            self.last_lengths = torch.cat([fp[2, n_evals - 1] for fp in fp_l])

            stats = torch.stack([cur_std.mean(), undiscounted_returns.mean(), undiscounted_returns.std(unbiased=False),
                                 undiscounted_returns.max(), undiscounted_returns.min(), fs.mean(),
                                 first_path[2].to(torch.float64).mean()])
            host = torch.cat([stats, cur_mean, cur_std]).cpu().numpy()          # the iteration's one host read
            P = cur_mean.numel()
            logger.push_prefix('itr #%d | ' % itr)
            logger.record_tabular('Iteration', itr)
            logger.record_tabular('CurStdMean', host[0])
            logger.record_tabular('AverageReturn', host[1])
            logger.record_tabular('StdReturn', host[2])
            logger.record_tabular('MaxReturn', host[3])
            logger.record_tabular('MinReturn', host[4])
            logger.record_tabular('AverageDiscountedReturn', host[5])
            logger.record_tabular('NumTrajs', n_used)
            logger.record_tabular('AvgTrajLen', host[6])

            policy.set_param_values(best_x)
            if self.record_paths:
                paths = self._first_paths(traj_l, fp_l, n_used)
                self.env.log_diagnostics(paths)
                policy.log_diagnostics(paths)
            logger.save_itr_params(itr, dict(
                itr=itr,
                policy=policy,
                env=self.env,
                cur_mean=host[7:7 + P].copy(),
                cur_std=host[7 + P:].copy(),
            ))
            logger.dump_tabular(with_prefix=False)
            logger.pop_prefix()
        vec_env.terminate()

    @staticmethod
    def _first_paths(traj_l, fp_l, n_used):
        """``PathList`` over the first path of every evaluation of the ``n_used`` candidates counted (cem.py:163): the
        launches' planes side by side, valid = the steps of each env's first path."""
        from rllab_amd.sampler.trajectories import PathList, Trajectories
        valid, start = [], 0
        for traj, fp in zip(traj_l, fp_l):
            n_evals, n_cand = fp.shape[1], fp.shape[2]
            t = torch.arange(traj.T, device=traj.device).view(-1, 1, 1)
            used = (start + torch.arange(n_cand, device=traj.device)) < n_used
            valid.append(((t < fp[2].view(1, n_evals, n_cand)) & used.view(1, 1, -1)).reshape(traj.T, -1))
            start += n_cand
        if len(traj_l) == 1:
            traj = traj_l[0]
        else:
            cat = lambda name, dim: torch.cat([getattr(c, name) for c in traj_l], dim=dim)
            traj = Trajectories(cat("obs", 2), cat("actions", 2), cat("means", 2), None, cat("rewards", 1), cat("dones", 1),
                                traj_l[0].max_path_length, log_std_planes=cat("log_std_planes", 2),
                                prev_action_info=traj_l[0].prev_action_info)
        traj.valid = torch.cat(valid, dim=1)
        return PathList(traj)
