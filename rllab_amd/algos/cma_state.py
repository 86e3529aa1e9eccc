"""The search distribution of CMA-ES: the default-option path of rllab/algos/cma_es_lib.py (CMAEvolutionStrategy with
``CMA_active``, cumulative step-size adaptation, lazy eigendecomposition, the stop criteria), restated on float64 tensors
of any device.

``CMAState(x0, sigma0, options)`` has ``ask(number=None)``, ``tell(xs, fs)``, ``stop()`` and ``result()``.  Everything of
size N or N x N (mean, pc, ps, C, B, D, the negative accumulator ``_Yneg``, the best-ever point) lives on the device of
``x0``; counters and the short fitness histories live on the host.  ``tell`` and ``ask`` read nothing back: the decisions the
library takes on host floats (hsig, the clip of the log step, the minstd / maxstd / mindx guards, the sigma rescale, the
choice between the plain and the clipped negative update) are ``torch.where`` on device scalars.  What the host does need --
the stop inputs, the histories, the count of clipped updates -- is gathered in ONE small tensor (``report_tensor``) and
read once per ``stop()``.

The two N x N updates of ``tell`` (cma_es_lib.py:3808-3814) are one launch of ``rl_cmaes_cov_update`` on a HIP device and
``cov_update_torch`` -- the same arithmetic in torch, also the kernel's test definition -- elsewhere.

Deliberately not built (each raises or stops instead of going on silently):
  * bounds and penalties, geno-pheno transforms, injections, mirrors (``popsize`` < 6 asks the library for mirrors and is
    refused), TPA, ``repair_genotype`` (every told point was asked), ``CMA_diagonal``, noise handling, the data logger;
  * the geno-pheno transform the library introduces at max D / min D > 1e6 (:4099) and its coordinate rescale at
    max dC / min dC > 1e8 (:4079): the state stops with ``conditioncov`` there.
"""
import math

import numpy as np
import torch

import rllab_amd.misc.logger as logger

# defaults of cma_es_lib.py:4332-4391 that this path reads
DEFAULT_OPTIONS = dict(
    popsize=None,            # 4 + int(3 * log(N))
    CMA_active=True,
    updatecovwait=None,
    maxiter=None,            # 100 + 50 * (N + 3) ** 2 // popsize ** 0.5
    maxfevals=float("inf"),
    ftarget=-float("inf"),
    tolx=1e-11,
    tolfacupx=1e3,
    tolfun=1e-11,
    tolfunhist=1e-12,
    tolstagnation=None,      # int(100 + 100 * N ** 1.5 / popsize)
    tolupsigma=1e20,
    minstd=0.0,
    maxstd=float("inf"),
    mindx=0.0,
    seed=None,
)

CLIP_FAC = 0.60              # cma_es_lib.py:4016
FLAT_FITNESS_KEY = "flat fitness: please (re)consider how to compute the fitness more elaborate"     # the library's key, :4926

_EIGH_PATH = {}              # device type -> "torch" | "numpy" (decided once per process)


class CMAParameters(object):
    """``_CMAParameters.set`` (cma_es_lib.py:4998-5124) and ``CMAAdaptSigmaCSA.initialize`` (:2218-2227) with the default
    options: host floats and float64 numpy weight vectors."""

    def __init__(self, N, popsize=None, active=True):
        N = int(N)
        if popsize is None:
            popsize = 4 + int(3 * math.log(N))
        popsize = int(popsize)
        if popsize < 6:
            # 'CMA_mirrors': 'popsize < 6' (:4339) turns mirrored sampling on
            raise NotImplementedError("CMAState: popsize=%d < 6 asks the library for mirrored samples, which are not built" % popsize)
        self.N, self.popsize = N, popsize
        self.lam_mirr = 0                                             # int(0.5 + CMA_mirrors * popsize), CMA_mirrors False (:5022)
        self.mu = max(int(0.5 * popsize + 0.499999), 1)               # :5033-5037
        w = np.log(max(self.mu, popsize / 2.0) + 0.5) - np.log(1 + np.arange(self.mu))      # :5047
        self.weights = w / np.sum(w)
        self.mueff = 1 / np.sum(self.weights ** 2)
        self.cs = (self.mueff + 2) / (N + (self.mueff + 3))           # :2221
        self.cc = (4 + self.mueff / N) / (N + (4 + 2 * self.mueff / N))                     # :5059-5061
        self.c1 = min(1, popsize / 6) * 2 / ((N + 1.3) ** 2.0 + self.mueff)                 # :5069-5071
        self.cmu = min(1 - self.c1, 2.0 * (0.3 + self.mueff - 2 + 1 / self.mueff) /
                       ((N + 2) ** 2.0 + 2.0 * self.mueff / 2))       # :5076-5079 (CMA_rankmualpha = 0.3)
        if active:
            ks = np.arange(np.ceil(popsize / 2 + 1.1 / 2), popsize + .1)
            wn = np.array([np.log(k) - np.log(popsize / 2 + 1 / 2) for k in ks])        # :5094
            self.neg_mu = len(wn)
            self.neg_weights = wn / np.sum(wn)
            self.neg_mueff = 1 / np.sum(self.neg_weights ** 2)
            self.neg_cmuexp = 0.3 * self.neg_mueff / ((N + 2) ** 1.5 + 1.0 * self.neg_mueff)    # :5099
        else:
            self.neg_mu, self.neg_weights, self.neg_mueff, self.neg_cmuexp = 0, np.zeros(0), 0.0, 0
        self.damps = (0.5 + 0.5 * min(1, (self.lam_mirr / (0.159 * popsize) - 1) ** 2) +
                      2 * max(0, ((self.mueff - 1) / (N + 1)) ** 0.5 - 1) + self.cs)        # :2222-2226
        self.cmean = 1.0
        self.chiN = N ** 0.5 * (1 - 1. / (4. * N) + 1. / (21. * N ** 2))                    # :2899

    def as_dict(self):
        return dict(popsize=self.popsize, mu=self.mu, neg_mu=self.neg_mu, lam_mirr=self.lam_mirr, mueff=self.mueff,
                    cs=self.cs, cc=self.cc, c1=self.c1, cmu=self.cmu, neg_mueff=self.neg_mueff, neg_cmuexp=self.neg_cmuexp,
                    damps=self.damps, cmean=self.cmean, chiN=self.chiN, weights=self.weights,
                    neg_weights=self.neg_weights)


def cov_update_torch(C, Yneg, dC, Ypos, wpos, Vneg, wneg, pc, scal):
    """The two matrix updates of ``tell`` in place (cma_es_lib.py:3808-3814), ``scal`` = [1 - c1a - cmu, c1, 1 - cmuexp]:

        _Yneg <- scal[2] * _Yneg + sum_k wneg[k] Vneg[k] Vneg[k]^T - C_old        (skipped when ``Yneg`` is None)
        C     <- scal[0] * C_old + sum_k wpos[k] Ypos[k] Ypos[k]^T + scal[1] pc pc^T
        dC    <- diag(C)

    The definition ``rl_cmaes_cov_update`` is tested against, and what runs where there is no HIP device."""
    if Yneg is not None:
        Yneg.mul_(scal[2])
        Yneg.add_(torch.matmul(wneg * Vneg.t(), Vneg) - C)
    C.mul_(scal[0])
    C.add_(torch.outer(scal[1] * pc, pc) + torch.matmul(wpos * Ypos.t(), Ypos))
    dC.copy_(torch.diagonal(C))


def cov_update_hip(C, Yneg, dC, Ypos, wpos, Vneg, wneg, pc, scal, N=None):
    """``rl_cmaes_cov_update`` on the tensors' device: one pass over ``C`` and ``_Yneg`` (row stride = their stride(0), so
    the N x N corner of a padded allocation works), Ypos [mu][N] / Vneg [mu_neg][N] contiguous."""
    from rllab_amd import _lib
    N = int(C.shape[0] if N is None else N)
    assert C.dtype == torch.float64 and C.stride(1) == 1 and scal.dtype == torch.float64 and scal.numel() >= 3
    mu, mu_neg = int(Ypos.shape[0]), (0 if Yneg is None else int(Vneg.shape[0]))
    assert Ypos.is_contiguous() and Ypos.shape[1] == N and wpos.numel() == mu and pc.numel() == N and dC.numel() >= N
    if Yneg is not None:
        assert Yneg.dtype == torch.float64 and Yneg.stride() == C.stride() and Vneg.is_contiguous() and wneg.numel() == mu_neg
        assert mu_neg == 0 or Vneg.shape[1] == N
    p = lambda t: None if t is None else _lib.ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib.rl_cmaes_cov_update(
        N, int(C.stride(0)), mu, mu_neg, p(C), p(Yneg), p(dC), p(Ypos), p(wpos.contiguous()),
        p(Vneg) if (Yneg is not None and mu_neg) else None, p(wneg.contiguous()) if (Yneg is not None and mu_neg) else None,
        p(pc.contiguous()), p(scal), _lib.stream_ptr(C.device)), "rl_cmaes_cov_update")


def _eigh_numpy(C):
    w, V = np.linalg.eigh(C.cpu().numpy())
    return torch.as_tensor(w, device=C.device), torch.as_tensor(V, device=C.device)


def eigh(C):
    """(eigenvalues ascending, eigenvectors in columns) of a symmetric float64 matrix on its own device
    (``torch.linalg.eigh``).  The first call per device type checks the device solver once on the matrix at hand
    (residual and orthogonality against 1e-10, one host read); where it is missing or wrong every call goes through
    ``numpy.linalg.eigh`` on the host with one copy each way, said once in the log."""
    kind = C.device.type
    path = _EIGH_PATH.get(kind)
    if path is None:
        path, why = "torch", None
        if kind != "cpu":
            try:
                w, V = torch.linalg.eigh(C)
                scale = float(C.abs().max()) or 1.0
                res = float((torch.matmul(V * w, V.t()) - C).abs().max()) / scale
                orth = float((torch.matmul(V.t(), V) - torch.eye(C.shape[0], dtype=C.dtype, device=C.device)).abs().max())
                if not (res <= 1e-10 and orth <= 1e-10):
                    path, why = "numpy", "residual %.2e, orthogonality %.2e" % (res, orth)
            except RuntimeError as e:        # no float64 solver in this build
                path, why = "numpy", str(e).splitlines()[0]
        if path == "numpy":
            logger.log("CMAState: torch.linalg.eigh is not usable in float64 on %s (%s); eigendecompositions run in "
                       "numpy.linalg.eigh on the host" % (kind, why))
        _EIGH_PATH[kind] = path
    if path == "numpy":
        return _eigh_numpy(C)
    return torch.linalg.eigh(C)


def eigh_path(device):
    """"torch" / "numpy" once ``eigh`` has run on a tensor of this device type, else None."""
    return _EIGH_PATH.get(torch.device(device).type)


class CMAState(object):
    # report_tensor(): the fixed head, then three values per tell not yet read
    R_SIGMA, R_MAXD, R_MIND, R_TOLUPSIGMA, R_TOLX, R_TOLFACUPX, R_NOEFFECTCOORD, R_NOEFFECTAXIS, R_COND, R_NOTPOSDEF, \
        R_CLIPPED, R_BESTF, R_BESTEVALS, R_HEAD = range(14)

    def __init__(self, x0, sigma0, options=None):
        opts = dict(DEFAULT_OPTIONS)
        for k, v in (options or {}).items():
            if k not in opts:
                raise TypeError("CMAState: unknown option %r (known: %s)" % (k, ", ".join(sorted(opts))))
            opts[k] = v
        x0 = torch.as_tensor(x0)
        self.device = x0.device
        self.f64 = dict(dtype=torch.float64, device=self.device)
        self.mean = x0.detach().to(torch.float64).reshape(-1).clone()
        N = self.N = int(self.mean.numel())
        if N <= 1:
            raise ValueError("optimization in 1-D is not supported")          # :2949
        self.sp = sp = CMAParameters(N, opts["popsize"], bool(opts["CMA_active"]))
        if opts["maxiter"] is None:
            opts["maxiter"] = 100 + 50 * (N + 3) ** 2 // sp.popsize ** 0.5
        if opts["tolstagnation"] is None:
            opts["tolstagnation"] = int(100 + 100 * N ** 1.5 / sp.popsize)
        self.opts = opts
        self.sigma0 = float(sigma0)
        t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64), **self.f64)
        self.sigma = t(self.sigma0)
        self.tolupsigma = t(opts["tolupsigma"])                       # divided by alpha ** 0.5 at a sigma rescale (:3849)
        self.weights, self.neg_weights = t(sp.weights), t(sp.neg_weights)
        self.wpos = t(sp.cmu * sp.weights)                            # "learning rate integrated" (:3801)
        self.pc = torch.zeros(N, **self.f64)
        self.ps = torch.zeros(N, **self.f64)
        self.B = torch.eye(N, **self.f64)
        self.dC = torch.exp((1e-4 / N) * torch.arange(N, **self.f64))                       # :2867
        self.C = torch.diag(self.dC)
        self.D = self.dC ** 0.5
        self._Yneg = torch.zeros((N, N), **self.f64) if sp.neg_cmuexp else None
        self.scal = torch.zeros(4, **self.f64)                        # the kernel's scalar block
        self.mean_old = self.mean
        self.countiter = self.countevals = self.itereigenupdated = 0
        self._count_eigen_host = 0
        self._clipped = torch.zeros((), **self.f64)                   # clipped negative updates: one more eigendecomposition each (:4053)
        self._cond = torch.zeros((), **self.f64)                      # a transform the library would introduce: conditioncov
        self._notposdef = torch.zeros((), **self.f64)
        self._clipped_host = 0
        self.best_x = torch.full((N,), float("nan"), **self.f64)
        self.best_f = t(float("inf"))
        self.best_evals = t(0.0)
        self.fit_hist, self.fit_histbest, self.fit_histmedian = [], [], []
        self._fit_first = self._fit_last = None
        self._pending = []                                            # per tell not yet read: [fit[0], median entry, fit[-1]]
        self._pending_iters = []
        self.last_z = None
        self._stopdict = {}
        seed = opts["seed"]
        self.gen = torch.Generator(device=self.device)
        if seed is None:
            self.gen.seed()
        else:
            self.gen.manual_seed(int(seed))
        self._told = True

    # ---------------------------------------------------------------------------------------------- sampling
    def _eigen_due(self):
        """The lazy criterion of ask_geno (cma_es_lib.py:3124-3134)."""
        sp, wait, gap = self.sp, self.opts["updatecovwait"], self.countiter - self.itereigenupdated
        return ((wait is None and self.countiter >= self.itereigenupdated + 1. / (sp.c1 + sp.cmu) / self.N / 10) or
                (wait is not None and self.countiter > self.itereigenupdated + wait) or
                (sp.neg_cmuexp * gap > 0.5))

    def ask(self, number=None):
        """``number`` (default popsize) candidates [number, N]:  mean + sigma * (B (D o z)),  z ~ N(0, I) kept in
        ``last_z`` (ask_geno, :3096-3251).  Updates B and D first when the lazy criterion says so."""
        if number is None or number < 1:
            number = self.sp.popsize
        if self._eigen_due():
            self.updateBD()
        arz = torch.randn((int(number), self.N), generator=self.gen, **self.f64)
        ary = torch.matmul(self.B, (self.D * arz).t()).t()             # :3216
        self.last_z = arz
        self._told = False
        return self.mean + self.sigma * ary

    def decompose_C(self):
        """Symmetrise, eigh, sqrt, ascending sort (:3967-3999)."""
        self.C = (self.C + self.C.t()) / 2
        self.dC = torch.diagonal(self.C).clone()
        w, self.B = eigh(self.C)
        self._notposdef = torch.maximum(self._notposdef, (w <= 0).any().to(torch.float64))
        D = w ** 0.5
        idx = torch.sort(D, stable=True).indices
        self.D, self.B = D[idx], self.B[:, idx]
        self._count_eigen_host += 1

    def updateBD(self):
        """cma_es_lib.py:4000-4121: the pending negative update in one of its three forms, then the decomposition."""
        if self.itereigenupdated == self.countiter:
            return
        sp, N = self.sp, self.N
        if sp.neg_cmuexp:
            gap = self.countiter - self.itereigenupdated
            C_shrunken = (1 - sp.cmu - sp.c1) ** gap
            if gap * sp.neg_cmuexp * N < CLIP_FAC * C_shrunken:
                # pos.def. guaranteed, because vectors are normalized
                self.C -= sp.neg_cmuexp * self._Yneg
            else:
                # two additional eigendecompositions to guarantee pos.def. (:4037-4046)
                self.decompose_C()
                inv_root = torch.matmul(self.B / self.D, self.B.t())
                inv_root = (inv_root + inv_root.t()) / 2
                Zneg = torch.matmul(torch.matmul(inv_root, self._Yneg), inv_root)
                maxeig = eigh(Zneg)[0].max()
                self._count_eigen_host += 1
                clipped = maxeig * sp.neg_cmuexp > CLIP_FAC              # a device value: no host read decides the branch
                rate = torch.where(clipped, CLIP_FAC / maxeig, torch.full_like(maxeig, sp.neg_cmuexp))
                self.C -= rate * self._Yneg
                self._clipped = self._clipped + clipped.to(torch.float64)    # the library checks C with one more eigh (:4053)
            self._Yneg = torch.zeros((N, N), **self.f64)
        dC = torch.diagonal(self.C)
        self._cond = torch.maximum(self._cond, (dC.max() / dC.min() > 1e8).to(torch.float64))      # :4079, not built
        self.decompose_C()
        self._cond = torch.maximum(self._cond, (self.D.max() / self.D.min() > 1e6).to(torch.float64))   # :4099, not built
        self.itereigenupdated = self.countiter

    # ---------------------------------------------------------------------------------------------- update
    def mahalanobis_norm(self, dx):
        """:4272, rows of ``dx`` [k, N] -> [k]."""
        return torch.sqrt(((torch.matmul(dx, self.B) / self.D) ** 2).sum(dim=1)) / self.sigma

    def tell(self, xs, fs):
        """cma_es_lib.py:3612-3861 for points that were asked (``xs`` [lam, N], ``fs`` [lam], lam >= mu; weights and mu stay
        those of popsize however many are told)."""
        if self._told:
            raise RuntimeError("tell should only be called once per iteration")
        sp, N = self.sp, self.N
        xs = torch.as_tensor(xs).to(**self.f64)
        fs = torch.as_tensor(fs).to(**self.f64).reshape(-1)
        lam = int(xs.shape[0])
        if lam != fs.numel():
            raise ValueError("for each candidate solution a function value must be provided")
        if lam < 3:
            raise ValueError("population size %d is too small" % lam)
        if lam < sp.mu or lam < sp.neg_mu:
            raise ValueError("not enough solutions passed to function tell (mu>lambda)")
        self.countiter += 1
        self.countevals += sp.popsize                                  # :3638: popsize, whatever lam is
        idx = torch.sort(fs, stable=True).indices                      # np.argsort of distinct values; ties keep index order
        fit = fs[idx]
        # BestSolution.update (:833-846): the first minimum, kept when strictly better
        better = fit[0] < self.best_f
        self.best_x = torch.where(better, xs[idx[0]], self.best_x)
        self.best_f = torch.where(better, fit[0], self.best_f)
        self.best_evals = torch.where(better, (self.countevals - lam + 1 + idx[0]).to(torch.float64), self.best_evals)
        # fitness histories (:3669-3679) are host lists: queued here, appended at the next host read
        if lam < 21:
            med = fit[lam // 2] if lam % 2 else 0.5 * (fit[lam // 2 - 1] + fit[lam // 2])
        else:
            med = fit[sp.popsize // 2]
        self._pending.append(torch.stack([fit[0], med, fit[-1]]))
        self._pending_iters.append(self.countiter)

        pop = xs[idx]
        mold = self.mean_old = self.mean
        self.mean = mold + sp.cmean * (torch.matmul(self.weights, pop[:sp.mu]) - mold)      # :3761
        # hsig (:2148-2159) updates ps first (:2249-2262) with the B, D and sigma of the last iteration
        dm = self.mean - mold
        z = torch.matmul(self.B, (1. / self.D) * torch.matmul(self.B.t(), dm))
        z = z * (sp.mueff ** 0.5 / self.sigma / sp.cmean)
        self.ps = (1 - sp.cs) * self.ps + math.sqrt(sp.cs * (2 - sp.cs)) * z
        squared_sum = (self.ps ** 2).sum() / (1 - (1 - sp.cs) ** (2 * self.countiter))
        hsig = (squared_sum / N - 1 < 1 + 4. / (N + 1)).to(torch.float64)
        c1a = sp.c1 - (1 - hsig ** 2) * sp.c1 * sp.cc * (2 - sp.cc)      # adjust for variance loss (:3787)
        self.pc = (1 - sp.cc) * self.pc + hsig * (math.sqrt(sp.cc * (2 - sp.cc) * sp.mueff) / self.sigma / sp.cmean) * dm
        # covariance matrix adaptation (:3800-3814)
        Y = ((pop[:sp.mu] - mold) / self.sigma).contiguous()
        V = None
        if sp.neg_cmuexp:
            V = (pop[lam - sp.neg_mu:] - mold) / self.sigma
            # normalize to constant Mahalanobis length sqrt(N) with the CURRENT B and D (:3805-3807)
            V = (V * (N ** 0.5 / self.mahalanobis_norm(V) / self.sigma).unsqueeze(1)).contiguous()
        self.scal = torch.stack([1 - c1a - sp.cmu, torch.full_like(c1a, sp.c1), torch.full_like(c1a, 1 - sp.neg_cmuexp),
                                 self.sigma])
        if self.dC.data_ptr() == self.C.data_ptr() or not self.dC.is_contiguous():
            self.dC = self.dC.clone()
        update = cov_update_hip if self.C.is_cuda else cov_update_torch
        update(self.C, self._Yneg if sp.neg_cmuexp else None, self.dC, Y, self.wpos, V, self.neg_weights, self.pc, self.scal)
        # cumulative step-size adaptation (:2264-2277) with the +-1 clip of the log step
        s = (torch.sqrt((self.ps ** 2).sum()) / sp.chiN - 1) * (sp.cs / sp.damps)
        self.sigma = self.sigma * torch.exp(torch.clamp(s, -1.0, 1.0))
        # guards (:3834-3843)
        o = self.opts
        sd = self.dC ** 0.5
        self.sigma = torch.where(self.sigma * sd.min() < o["minstd"], o["minstd"] / sd.min(), self.sigma)
        self.sigma = torch.where(self.sigma * sd.max() > o["maxstd"], o["maxstd"] / sd.max(), self.sigma)
        self.sigma = torch.where(self.sigma * self.D.min() < o["mindx"], o["mindx"] / self.D.min(), self.sigma)
        # sigma > 1e9 sigma0: move the scale into C (:3845-3849); alpha = 1 (exact) otherwise
        alpha = torch.where(self.sigma > 1e9 * self.sigma0, self.sigma / self.D.max(), torch.ones_like(self.sigma))
        self.C *= alpha
        self.dC *= alpha
        self.D = self.D * alpha ** 0.5
        self.sigma = self.sigma / alpha ** 0.5
        self.tolupsigma = self.tolupsigma / alpha ** 0.5
        self._told = True

    # ---------------------------------------------------------------------------------------------- host side
    @property
    def count_eigen(self):
        self._sync()
        return self._count_eigen_host + self._clipped_host

    def report_tensor(self):
        """float64 [R_HEAD + 3 * (tells not yet read)] on the device: everything ``stop()`` needs from the device.  A
        caller that reads the host anyway appends it to its own read and hands the values to ``stop(report=...)``."""
        o, sd = self.opts, self.dC ** 0.5
        f = lambda b: b.to(torch.float64)
        tolx = f(((self.sigma * self.pc < o["tolx"]).all()) & ((self.sigma * sd < o["tolx"]).all()))       # :4859-4861
        tolfacupx = f((self.sigma * sd > self.sigma0 * o["tolfacupx"]).any())                                # :4862-4864
        # np.where(...)[0] then any(idx): an index list is "any" when it holds a NONZERO index (:4894-4896)
        coord = self.mean == self.mean + 0.2 * self.sigma * sd
        noeffectcoord = f(coord[1:].any())
        i = self.countiter % self.N
        noeffectaxis = f((self.mean == self.mean + 0.1 * self.sigma * self.D[i] * self.B[:, i]).sum() == self.N)
        head = torch.stack([self.sigma, self.D.max(), self.D.min(), self.tolupsigma, tolx, tolfacupx, noeffectcoord,
                            noeffectaxis, self._cond, self._notposdef, self._clipped, self.best_f, self.best_evals])
        return torch.cat([head] + self._pending)

    def _absorb(self, host):
        """Take a host copy of ``report_tensor()``: extend the histories (:3669-3679), keep the head."""
        host = np.asarray(host, dtype=np.float64)
        N, popsize = self.N, self.sp.popsize
        for k, it in enumerate(self._pending_iters):
            first, med, last = host[self.R_HEAD + 3 * k:self.R_HEAD + 3 * k + 3]
            self.fit_hist.insert(0, first)
            if it % 5 == 0:
                self.fit_histbest.insert(0, first)
                self.fit_histmedian.insert(0, med)
            if len(self.fit_histbest) > 2e4:
                self.fit_histbest.pop()
                self.fit_histmedian.pop()
            if len(self.fit_hist) > 10 + 30 * N / popsize:
                self.fit_hist.pop()
            self._fit_first, self._fit_last = first, last
        self._pending, self._pending_iters = [], []
        self._head = host[:self.R_HEAD].copy()
        self._clipped_host = int(round(self._head[self.R_CLIPPED]))
        if self._head[self.R_NOTPOSDEF]:
            raise ValueError("covariance matrix was not positive definite, this must be considered as a bug")   # :3992

    def _sync(self):
        self._absorb(self.report_tensor().cpu().numpy())

    def stop(self, report=None):
        """The dictionary of fired termination criteria (cma_es_lib.py:4827-4929), empty while none fires."""
        if self.countiter == 0:
            return {}
        if report is None:
            self._sync()
        else:
            self._absorb(report)
        h, o, N = self._head, self.opts, self.N
        hist, histbest, histmedian = self.fit_hist, self.fit_histbest, self.fit_histmedian
        d = {}

        def add(key, cond, val=None):
            if cond:
                d[key] = val if val is not None else o.get(key)
        add("ftarget", h[self.R_BESTF] < o["ftarget"])
        add("maxfevals", self.countevals - 1 >= o["maxfevals"])
        add("maxiter", self.countiter >= 1.0 * o["maxiter"])
        add("tolx", bool(h[self.R_TOLX]))
        add("tolfacupx", bool(h[self.R_TOLFACUPX]))
        add("tolfun", self._fit_last - self._fit_first < o["tolfun"] and max(hist) - min(hist) < o["tolfun"])
        add("tolfunhist", len(hist) > 9 and max(hist) - min(hist) < o["tolfunhist"])
        l = int(max((1.0 * o["tolstagnation"] / 5. / 2, len(histbest) / 10)))
        add("tolstagnation", o["tolstagnation"] and self.countiter > N * (5 + 100 / self.sp.popsize) and
            len(histbest) > 100 and 2 * l < len(histbest) and
            np.median(histmedian[:l]) >= np.median(histmedian[l:2 * l]) and
            np.median(histbest[:l]) >= np.median(histbest[l:2 * l]))
        add("tolupsigma", h[self.R_TOLUPSIGMA] and h[self.R_SIGMA] / h[self.R_MAXD] > self.sigma0 * h[self.R_TOLUPSIGMA],
            h[self.R_TOLUPSIGMA])
        add("noeffectcoord", bool(h[self.R_NOEFFECTCOORD]), True)
        add("noeffectaxis", bool(h[self.R_NOEFFECTAXIS]), True)
        add("conditioncov", h[self.R_MAXD] > 1e7 * h[self.R_MIND] or bool(h[self.R_COND]), 1e14)
        if len(d):
            add(FLAT_FITNESS_KEY, len(hist) > 9 and max(hist) == min(hist), True)
        self._stopdict = d
        return d

    def result(self):
        """(xbest, f(xbest), evaluations_xbest, evaluations, iterations, mean, effective stds) (:3888-3898); xbest, mean and
        the stds are tensors on the state's device."""
        self._sync()
        return (self.best_x, float(self._head[self.R_BESTF]), int(self._head[self.R_BESTEVALS]), self.countevals,
                self.countiter, self.mean, self.sigma * self.dC ** 0.5)
