"""The closures that NPO / VPG / REPS ``init_opt`` hand their optimizers, pinned on the host for the four update-batch
signatures (rllab_amd/policies/update_batch.py): tests/golden/update_closures.json holds every value as ``float.hex()``,
recorded by tools/make_golden_update_closures.py with the code of the commit its header names, float64 parameters on the
CPU, one thread.

Shapes: obs 3, 2 actions, hidden (4,), T = 5, N = 3.  Env 0's first path ends at t = 2 (``start`` has an interior True),
env 2's last two steps are cut from the batch (``weights`` has zeros), the advantages have both signs, and the old
distribution is far enough from the new one that likelihood ratios lie on either side of the truncation at 1.1 (asserted).

Every closure is evaluated twice: with what ``npo_inputs`` returns and with ``tuple(...)`` of it, which is what
ConjugateGradientOptimizer.optimize makes of it before any closure or ops method sees it.

Bound: |got - pin| <= 1e-12 max(1, |pin|).  The values are float64 sums of at most 15 x 2 terms; another summation order
moves them by at most n 2^-53 ~ 3e-15 of the sum of the terms' magnitudes, and |pin| is never more than that sum, so this
asks no less than 1e-12 max(1, sum |terms|) would.  On the machine that recorded them the values are equal."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_closures.json")
DO, DA, HIDDEN, T, N = 3, 2, 4, 5, 3
TRUNC = 1.1
FAMILIES = ("gaussian", "categorical", "recurrent_gaussian", "recurrent_categorical")
TIN = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 3, 3], [1, 4, 4]]             # env 0: a path ends at t = 2
VALID = [[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 0], [1, 1, 0]]           # env 2: the last two steps are not in the batch


class _Env(object):
    def __init__(self, spec):
        self.spec = spec
        self.observation_space, self.action_space = spec.observation_space, spec.action_space


class _NoSampler(object):
    def __init__(self, algo):
        pass


class _Recorder(object):
    """Stands where the optimizer does: keeps what ``init_opt`` hands over."""
    _subsample_factor = 1.0

    def update_opt(self, *args, **kw):
        self.args, self.kw = args, kw


class _Traj(object):
    """The fields of a processed dense batch that ``npo_inputs`` reads."""
    count = None
    log_std_planes = None


def _policy(family):
    from rllab_amd.envs.env_spec import EnvSpec
    from rllab_amd.spaces import Box, Discrete
    np.random.seed(0)
    if "categorical" in family:
        spec = EnvSpec(Discrete(DO), Discrete(DA))
    else:
        spec = EnvSpec(Box(-np.ones(DO), np.ones(DO)), Box(-np.ones(DA), np.ones(DA)))
    if family == "gaussian":
        from rllab_amd.policies.gaussian_mlp_policy import GaussianMLPPolicy
        pol = GaussianMLPPolicy(spec, hidden_sizes=(HIDDEN,))
    elif family == "categorical":
        from rllab_amd.policies.categorical_mlp_policy import CategoricalMLPPolicy
        pol = CategoricalMLPPolicy(spec, hidden_sizes=(HIDDEN,))
    elif family == "recurrent_gaussian":
        from rllab_amd.policies.gaussian_gru_policy import GaussianGRUPolicy
        pol = GaussianGRUPolicy(spec, hidden_sizes=(HIDDEN,))
    else:
        from rllab_amd.policies.categorical_gru_policy import CategoricalGRUPolicy
        pol = CategoricalGRUPolicy(spec, hidden_dim=HIDDEN)
    theta = pol.get_param_values()
    pol.set_param_values(theta + 0.3 * np.random.RandomState(1).randn(theta.size))
    pol.flat_params = pol.flat_params.detach().cpu().double()           # float64 parameters on the CPU
    return _Env(spec), pol


def _batch(family, pol):
    """A ``_Traj`` whose old distribution is the policy's own at parameters moved by 0.5 N(0, 1)."""
    rng = np.random.RandomState(2)
    cat = "categorical" in family
    tr = _Traj()
    tr.T, tr.N, tr.B, tr.obs_dim, tr.act_dim, tr.categorical = T, N, T * N, DO, DA, cat
    tr.tin = torch.tensor(TIN, dtype=torch.int32)
    tr.valid = torch.tensor(VALID, dtype=torch.bool)
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    if cat:
        tr.obs = f64(np.eye(DO)[rng.randint(0, DO, size=(T, N))].transpose(2, 0, 1))
        tr.actions = f64(np.eye(DA)[rng.randint(0, DA, size=(T, N))].transpose(2, 0, 1))
    else:
        tr.obs = f64(rng.randn(DO, T, N))
        tr.actions = f64(rng.randn(DA, T, N))
    tr.advantages = f64(rng.randn(T, N))
    old_flat = pol.flat_params + 0.5 * torch.as_tensor(rng.randn(pol.flat_params.numel()))
    with torch.no_grad():
        if pol.recurrent:
            old = pol.dist_info_planes(tr.obs, tr.actions, tr.tin == 0, old_flat)
        else:
            old = pol.dist_info_planes(tr.obs.reshape(DO, -1), old_flat)
    if cat:
        tr.means, tr.log_std = old["prob"].reshape(DA, T, N), None
    else:
        tr.means = old["mean"].reshape(DA, T, N)
        tr.log_std = old["log_std"].reshape(-1)[:DA] if pol.recurrent else old["log_std"].reshape(DA, -1)[:, 0]
        tr.log_std = tr.log_std.contiguous()
    return tr


def _algo(cls, env, pol, **kw):
    from rllab_amd.baselines.zero_baseline import ZeroBaseline
    from rllab_amd.misc import logger
    algo = cls(env=env, policy=pol, baseline=ZeroBaseline(env.spec), sampler_cls=_NoSampler, **kw)
    logger.set_quiet(True)
    try:
        algo.init_opt()
    finally:
        logger.set_quiet(False)
    return algo


def _value_grad(fn, pol, inputs):
    flat = pol.flat_params.detach().clone().requires_grad_(True)
    val = fn(flat, *inputs)
    (g,) = torch.autograd.grad(val, flat)
    return [float(val.detach())], [float(x) for x in g]


def ratios(family, pol, inputs):
    """Likelihood ratios of the valid samples at the current parameters (the quantity ``truncate_local_is_ratio`` clamps)."""
    keys = ("prob",) if "categorical" in family else ("mean", "log_std")
    old = dict(zip(keys, inputs[3:3 + len(keys)]))
    with torch.no_grad():
        new = pol.dist_info_planes(inputs[0], inputs[1], inputs[3 + len(keys)]) if pol.recurrent else \
            pol.dist_info_planes(inputs[0])
        lr = pol.distribution.likelihood_ratio_sym(inputs[1], old, new, axis=0)
    return lr[inputs[-2] > 0]


def run_family(family, plain):
    """{quantity: [floats]} of one family; ``plain``: the closures get ``tuple(npo_inputs(...))``."""
    from rllab_amd.algos.npo import NPO, npo_inputs
    from rllab_amd.algos.reps import REPS
    from rllab_amd.algos.vpg import VPG
    torch.set_num_threads(1)
    env, pol = _policy(family)
    inputs = npo_inputs(pol, dict(_traj=_batch(family, pol)))
    if plain:
        inputs = tuple(inputs)
    lr = ratios(family, pol, inputs)
    assert bool((lr > TRUNC).any()) and bool((lr < TRUNC).any()), "the truncation case is vacuous"
    assert bool((inputs[-2] == 0).any()) and bool((inputs[2] > 0).any()) and bool((inputs[2] < 0).any())
    out = {}
    for tag, trunc in (("", None), ("_truncated", TRUNC)):
        rec = _Recorder()
        _algo(NPO, env, pol, optimizer=rec, truncate_local_is_ratio=trunc)
        out["npo_surr_loss" + tag], out["npo_surr_loss%s_grad" % tag] = _value_grad(rec.kw["loss"], pol, inputs)
        if trunc is None:
            out["npo_mean_kl"], out["npo_mean_kl_grad"] = _value_grad(rec.kw["leq_constraint"][0], pol, inputs)
    rec = _Recorder()
    algo = _algo(VPG, env, pol, optimizer=rec)
    out["vpg_surr_obj"], out["vpg_surr_obj_grad"] = _value_grad(rec.args[0], pol, inputs)
    out["vpg_f_kl"] = [float(x) for x in algo.opt_info["f_kl"](inputs)]
    if family == "gaussian":
        algo = _algo(REPS, env, pol)
        wts = inputs[2].abs() + 0.25                      # REPS's sample weights ride in the advantages slot
        rin = inputs._replace(advantages=wts) if hasattr(inputs, "_replace") else inputs[:2] + (wts,) + inputs[3:]
        out["reps_loss"], out["reps_loss_grad"] = _value_grad(algo.opt_info["f_loss"], pol, rin)
        out["reps_f_kl"] = [float(algo.opt_info["f_kl"](rin))]
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["parent_commit"]) == 40 and sorted(g["cases"]) == sorted(FAMILIES)
    return g["cases"]


@pytest.mark.parametrize("plain", [False, True], ids=["named", "plain_tuple"])
@pytest.mark.parametrize("family", FAMILIES)
def test_closures_compute_what_the_parent_computed(family, plain, golden):
    got, want = run_family(family, plain), golden[family]
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        pins = [float.fromhex(h) for h in want[k]]
        assert len(got[k]) == len(pins), k
        for i, (a, b) in enumerate(zip(got[k], pins)):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), "%s %s[%d]: %r, recorded %r" % (family, k, i, a, b)


def test_signatures_are_tuples_with_these_fields():
    from rllab_amd.policies import update_batch as ub
    fields = {ub.GaussianBatch: ["obs", "actions", "advantages", "old_mean", "old_log_std", "weights", "inv_count"],
              ub.CategoricalBatch: ["obs", "actions", "advantages", "old_prob", "weights", "inv_count"],
              ub.RecurrentGaussianBatch: ["obs", "actions", "advantages", "old_mean", "old_log_std", "start", "weights",
                                          "inv_count"],
              ub.RecurrentCategoricalBatch: ["obs", "actions", "advantages", "old_prob", "start", "weights", "inv_count"]}
    for sig, want in fields.items():
        assert list(sig._fields) == want and issubclass(sig, tuple)
        assert list(sig._fields[-2:]) == ["weights", "inv_count"]
        assert sig.has_start == ("start" in want)
    assert ub.GaussianBatch.old_keys == ub.RecurrentGaussianBatch.old_keys == ("mean", "log_std")
    assert ub.CategoricalBatch.old_keys == ub.RecurrentCategoricalBatch.old_keys == ("prob",)
    for family, sig in zip(FAMILIES, (ub.GaussianBatch, ub.CategoricalBatch, ub.RecurrentGaussianBatch,
                                      ub.RecurrentCategoricalBatch)):
        env, pol = _policy(family)
        assert ub.signature_of(pol) is sig
        from rllab_amd.algos.npo import npo_inputs
        assert type(npo_inputs(pol, dict(_traj=_batch(family, pol)))) is sig
