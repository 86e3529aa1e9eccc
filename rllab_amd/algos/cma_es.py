"""CMA-ES (API and control flow of rllab/algos/cma_es.py:30-155).

Per iteration: ask the search distribution for candidates in parameter space, score every candidate by minus the
discounted return of one rollout, tell the distribution.  The reference evaluates one candidate at a time
(``sample_return``, :16-27) and keeps the distribution in a NumPy library on the host (``cma_es_lib.CMAEvolutionStrategy(x0,
sigma0)`` with all default options).  Here a whole population is ONE launch of the population rollout
(``HipVecEnv.rollout_population``, as CEM uses it) and the distribution is ``CMAState`` (rllab_amd/algos/cma_state.py): the
library's default-option path restated on float64 device tensors, its N x N update one HIP kernel
(``rl_cmaes_cov_update``).  One host read per iteration brings the logged values, the inputs of the stop criteria and
the mean.

Not built: what ``CMAState`` leaves out (bounds, transforms, injections, mirrors, TPA, CMA_diagonal, noise handling, the
data logger); where the library would introduce a geno-pheno transform (max D / min D > 1e6) the run stops with
``conditioncov``.
"""
import numpy as np
import torch

import rllab_amd.misc.logger as logger
from rllab_amd.algos.base import RLAlgorithm
from rllab_amd.algos.cem import CEM, cem_sample_prefix, population_launcher, population_why_unsupported
from rllab_amd.algos.cma_state import CMAState
from rllab_amd.core.serializable import Serializable
from rllab_amd.misc import ext

MAX_PARAMS = 8192


class CMAES(RLAlgorithm, Serializable):

    def __init__(
            self,
            env,
            policy,
            n_itr=500,
            max_path_length=500,
            discount=0.99,
            sigma0=1.,
            batch_size=None,
            plot=False,
            popsize=None,
            seed=None,
            record_paths=True,
            updatecovwait=None,
            active=True,
            **kwargs
    ):
        """
        :param n_itr: Number of iterations.
        :param max_path_length: Maximum length of a single rollout.
        :param batch_size: # of samples from trajs from param distribution, when this
        is set, n_samples is ignored
        :param discount: Discount.
        :param plot: Plot evaluation run after each iteration.
        :param sigma0: Initial std for param dist
        :param popsize: engine option -- population size (None: the library's 4 + int(3 ln N))
        :param seed: engine option -- seed of the candidate draws and of the envs' Philox streams (None: ext.get_seed())
        :param record_paths: engine option -- False: no trajectory plane is stored and env / policy log_diagnostics are skipped
        :param updatecovwait: engine option -- the library's option of the same name: iterations without an update of B and D
        :param active: engine option -- the library's CMA_active (negative update of the covariance matrix)
        """
        Serializable.quick_init(self, locals())
        self.env = env
        self.policy = policy
        self.plot = plot
        self.sigma0 = sigma0
        self.discount = discount
        self.max_path_length = max_path_length
        self.n_itr = n_itr
        self.batch_size = batch_size
        self.popsize = popsize
        self.seed = seed
        self.record_paths = record_paths
        self.updatecovwait = updatecovwait
        self.active = active
        # the latest iteration's population, on the device (as CEM keeps it), the strategy, and per iteration the best
        # candidate told: (fitness, parameters)
        self.last_n_candidates = self.last_xs = self.last_fs = self.last_lengths = None
        self.es = None
        self.iteration_best = []
        self.stop_dict = {}

    def why_unsupported(self):
        """One sentence naming what keeps this configuration off the population rollout / the device-resident strategy, or None."""
        # the size first: no policy the population kernel runs today reaches it, a larger one must not get past it later
        n = int(self.policy.get_param_values().size) if hasattr(self.policy, "get_param_values") else 0
        if n > MAX_PARAMS:
            return ("%d parameters, more than %d: the three N x N float64 matrices of the full-covariance strategy would pass "
                    "1.6 GB" % (n, MAX_PARAMS))
        return population_why_unsupported(self.env, self.policy, self.plot)

    def train(self):
        reason = self.why_unsupported()
        if reason is not None:
            raise NotImplementedError("CMAES: " + reason)
        policy = self.policy
        dev = policy.flat_params.device
        seed = self.seed if self.seed is not None else ext.get_seed()
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        mpl = int(self.max_path_length)

        cur_std = self.sigma0
        cur_mean = torch.as_tensor(policy.get_param_values(), dtype=torch.float64, device=dev)
        es = self.es = CMAState(cur_mean, cur_std, dict(popsize=self.popsize, seed=int(seed), updatecovwait=self.updatecovwait,
                                                       CMA_active=bool(self.active)))
        P = es.N
        # candidates of one launch: the population, or what batch_size needs if every path runs full length
        n_launch = es.sp.popsize if self.batch_size is None else max(-(-int(self.batch_size) // mpl), 1)
        vec_env = self.env.vec_env_executor(n_envs=n_launch, max_path_length=mpl, seed=int(seed))
        launch = population_launcher(policy, vec_env)
        self.iteration_best, self.stop_dict = [], {}

        itr = 0
        while itr < self.n_itr and not self.stop_dict:
            xs_l, fp_l, traj_l, n_used = [], [], [], None
            while n_used is None:
                # Sample from multivariate normal distribution: every launch of one iteration from the same distribution
                xs = es.ask(n_launch)
                traj, first_path = launch(xs, 1, mpl, self.discount, bool(self.record_paths))
                xs_l.append(xs)
                fp_l.append(first_path.view(3, 1, n_launch))
                traj_l.append(traj)
                if self.batch_size is None:
                    n_used = n_launch
                else:
                    # paths count in index order until their lengths reach batch_size (cma_es.py:104-110)
                    n_used = cem_sample_prefix(torch.cat([fp[2, 0] for fp in fp_l]), self.batch_size)
            xs = torch.cat(xs_l)[:n_used]
            first_path = torch.cat(fp_l, dim=2)[:, 0, :n_used].to(torch.float64)        # [3, n_used]
            # Evaluate fitness of samples (negative as it is minimization problem).
            fs = -first_path[0]
            undiscounted_returns = first_path[1]
            # Update CMA-ES params based on sample fitness.
            es.tell(xs, fs)
            self.last_n_candidates, self.last_xs, self.last_fs = n_used, xs, fs
            self.last_lengths = torch.cat([fp[2, 0] for fp in fp_l])
            i_best = torch.sort(fs, stable=True).indices[0]
            self.iteration_best.append((fs[i_best], xs[i_best]))

            stats = torch.stack([undiscounted_returns.mean(), undiscounted_returns.max(), undiscounted_returns.min(),
                                 fs.mean(), first_path[2].mean()])
            report = es.report_tensor()
            host = torch.cat([stats, report, es.mean]).cpu().numpy()                    # the iteration's one host read
            rep = host[5:5 + report.numel()]
            self.stop_dict = es.stop(report=rep)

            logger.push_prefix('itr #%d | ' % itr)
            logger.record_tabular('Iteration', itr)
            logger.record_tabular('CurStdMean', np.mean(cur_std))          # the reference logs sigma0 every iteration (:123)
            logger.record_tabular('AverageReturn', host[0])
            logger.record_tabular('StdReturn', host[0])                    # ... and the mean under this name (:128-129)
            logger.record_tabular('MaxReturn', host[1])
            logger.record_tabular('MinReturn', host[2])
            logger.record_tabular('AverageDiscountedReturn', host[3])
            logger.record_tabular('AvgTrajLen', host[4])
            logger.record_tabular('Sigma', rep[CMAState.R_SIGMA])
            logger.record_tabular('AxisRatio', rep[CMAState.R_MAXD] / rep[CMAState.R_MIND])
            logger.record_tabular('NumTrajs', n_used)
            if self.stop_dict:
                logger.record_tabular('Stop', "|".join(sorted(self.stop_dict)))
                logger.log("CMAES: stopping on %r" % (self.stop_dict,))

            # the best-ever evaluated candidate: what result()[0] is, what the snapshot carries
            policy.set_param_values(es.best_x)
            if self.record_paths:
                paths = CEM._first_paths(traj_l, fp_l, n_used)
                self.env.log_diagnostics(paths)
                policy.log_diagnostics(paths)
            logger.save_itr_params(itr, dict(
                itr=itr,
                policy=policy,
                env=self.env,
                cur_mean=host[5 + report.numel():5 + report.numel() + P].copy(),
                sigma=float(rep[CMAState.R_SIGMA]),
            ))
            logger.dump_tabular(with_prefix=False)
            logger.pop_prefix()
            # Update iteration.
            itr += 1

        # Set final params.
        if es.countiter:
            policy.set_param_values(es.result()[0])
        vec_env.terminate()
