"""The seeds every acquisition path draws, their order, which of them pass through ``shard.agree``, and where the two global
generators stand afterwards - pinned for ``recommend``, ``acquisition_values`` and ``joint_acquisition_value`` of every path the
recommender serves, over the CPU doubles.

The draws come from torch's global generator and decide the recommendation, so their order is behaviour.  ``EXPECTED`` was
recorded by running ``_collect`` on commit 962bac3 (the parent of the change that gave every path one scorer surface,
``baybe_amd.scoring``), never from the code under test.

The forest, linear, qEHVI and qNIPV paths have no CPU double of their device calls; ``_SurfaceEngine`` gives them stand-ins (scores
that depend on the operands and the base samples, nothing more): what is pinned is the host layer's draw order, not their values.
"""

import sys

import numpy as np
import pytest
import torch

import _desirability_cases as dc
import _objective_cases as oc
import _oracle_desirability as od
import _oracle_ehvi as oe
import _oracle_nipv as on
from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, ParetoObjective, SearchSpace, SingleTargetObjective

REFUSALS = ("IncompatibilityError", "IncompatibleAcquisitionFunctionError", "IncompatibleSurrogateError")


class _SurfaceEngine(od.DesirabilityOracleEngine):
    """The oracle engine plus stand-ins for the device calls of the paths that have no CPU double."""

    forest = None
    n_trees = 4

    def _torch(self):
        return torch

    def ehvi_acq(self, log, mean, var, cells, z, alive=None, cross=None, stats=None, form=-1):
        lo, up = cells
        if cross is None:
            return self._mask(oe.q1_scores(log, mean.numpy(), var.numpy(), z, lo, up), alive)
        mp, cpp = stats
        return torch.from_numpy(oe.joint_scores(log, mean.numpy(), var.numpy(), cross.numpy(), mp, cpp, z, lo, up,
                                                alive=None if alive is None else alive.numpy()))

    def nipv_set_points(self, P):
        self._P = np.ascontiguousarray(P, dtype=np.float64)
        return on.schur(self._model, self._P[:1], None, self._P).var_p

    def nipv_gain(self, X, var, cross, H, ginv, alive=None):
        return self._mask(on.direct(self._model, self._np(X), self._pend, self._P).gain, alive)

    def forest_predict(self, forest, X):
        return self.posterior(X)[0][None, :].repeat(self.n_trees, 1)

    def predict(self, X):
        return self.forest_predict(None, X)

    def forest_mc_acq(self, forest, kind, X, counts, order, S, pend, best_f, sign, beta, alive=None):
        mean, var = self.posterior(X)
        spread = 0.0 if pend is None else float(pend.sum())
        return self._mask(sign * mean.numpy() + 1e-3 * float(counts[0]) * var.numpy() - 1e-6 * spread, alive)


def _install(monkeypatch):
    import _oracle_nei
    import _oracle_nparego
    from baybe_amd import engine as engine_mod
    from baybe_amd.surrogates import HipGaussianProcessSurrogate

    od.install(monkeypatch)
    _oracle_nparego.install(monkeypatch)
    _oracle_nei.install(monkeypatch)
    monkeypatch.setattr(engine_mod, "HipGP", _SurfaceEngine)
    forest = type("FakeForestSurrogate", (HipGaussianProcessSurrogate,), {"is_ensemble": True})
    linear = type("FakeLinearSurrogate", (HipGaussianProcessSurrogate,), {"is_independent_gaussian": True})
    return forest, linear


def _problem():
    """12 measurements, 40 candidates, d = 3."""
    rng = np.random.default_rng(5)
    space = SearchSpace.from_product([NumericalDiscreteParameter("x0", np.arange(5) / 4.0),
                                      NumericalDiscreteParameter("x1", np.arange(4) / 3.0),
                                      NumericalDiscreteParameter("x2", np.arange(2) / 1.0)])
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), 12, replace=False)].copy()
    X = meas[["x0", "x1", "x2"]].to_numpy(float)
    meas["y"] = -((X - 0.25) ** 2).sum(1) + 0.05 * rng.standard_normal(12)
    meas["t1"] = 1.0 - ((X - 0.3) ** 2).sum(1) + 0.02 * rng.standard_normal(12)
    meas["t2"] = ((X - 0.6) ** 2).sum(1) + 0.02 * rng.standard_normal(12)
    return space, exp, meas


def _paths(forest, linear):
    """name -> (recommender keywords, objective, batch size)."""
    from baybe_amd import acquisition as A

    single = SingleTargetObjective(NumericalTarget("y"))
    pareto = ParetoObjective([NumericalTarget("t1"), NumericalTarget("t2", minimize=True)])
    ramps = dc.DesirabilityObjective([dc.ramp_target("t1", 0.0, 1.2), dc.ramp_target("t2", 0.0, 1.5, descending=True)], weights=[2.0, 1.0])
    affine = dc.DesirabilityObjective([oc.affine_target("t1", 1.0, 0.0), oc.affine_target("t2", 1.0, 0.0, minimize=True)], scalarizer="MEAN")
    mc = dict(n_mc_samples=32)
    return {
        "single-mc": (dict(acquisition_function=A.qLogEI(**mc)), single, 2),
        "single-analytic": (dict(acquisition_function="EI"), single, 1),
        "transformed": (dict(acquisition_function=A.qLogEI(**mc)), SingleTargetObjective(oc.bell_target("y", -0.2, 0.3)), 2),
        "qNEI": (dict(acquisition_function=A.qNEI(**mc)), single, 2),
        "qLogNEI": (dict(acquisition_function=A.qLogNEI(**mc)), single, 2),
        "qLogNEHVI": (dict(acquisition_function=A.qLogNEHVI(**mc)), pareto, 2),
        "qNEHVI": (dict(acquisition_function=A.qNEHVI(**mc)), pareto, 2),
        "qLogNParEGO-drawn": (dict(acquisition_function=A.qLogNParEGO(**mc)), pareto, 2),
        "qLogNParEGO-given": (dict(acquisition_function=A.qLogNParEGO(scalarization_weights=[0.3, 0.7], **mc)), pareto, 2),
        "qLogEHVI": (dict(ehvi="device", acquisition_function=A.qLogEHVI(**mc)), pareto, 2),
        "qNIPV": (dict(nipv="device", acquisition_function=A.qNIPV(sampling_n_points=6)), single, 2),
        "desirability-mc": (dict(desirability="device", acquisition_function=A.qLogEI(**mc)), ramps, 2),
        "desirability-analytic": (dict(desirability="device", acquisition_function="EI"), affine, 1),
        "forest-mc": (dict(surrogate_model=forest(), acquisition_function=A.qLogEI(**mc)), single, 2),
        "linear-mc": (dict(surrogate_model=linear(), acquisition_function=A.qLogEI(**mc)), single, 1),
    }


def _one_rank_shard(n, agree):
    """A ``RowShard`` of one rank without a process group: the gathers return the local payload, ``agree`` records its calls."""
    from baybe_amd.distributed import RowShard

    class OneRank(RowShard):
        def _all_gather(self, payload):
            return payload.reshape(1, -1)

        def _payload_to_backend(self, payload_host, device):
            return torch.from_numpy(np.ascontiguousarray(payload_host, dtype=np.float64))

    shard = OneRank(n, rank=0, world=1)
    shard.agree = agree
    return shard


PATH_NAMES = ("single-mc", "single-analytic", "transformed", "qNEI", "qLogNEI", "qLogNEHVI", "qNEHVI", "qLogNParEGO-drawn",
              "qLogNParEGO-given", "qLogEHVI", "qNIPV", "desirability-mc", "desirability-analytic", "forest-mc", "linear-mc")


def _collect(name, monkeypatch):
    """{(pending?, sharded?, call): (seeds drawn, what passed through ``agree``, the generators' next draws or the refusal)}."""
    forest, linear = _install(monkeypatch)
    import baybe_amd.desirability, baybe_amd.ehvi, baybe_amd.forest, baybe_amd.linear, baybe_amd.nei, baybe_amd.nipv  # noqa: E401, F401
    import baybe_amd.nparego  # noqa: F401
    from baybe_amd import engine as engine_mod
    from baybe_amd.recommenders import HipBotorchRecommender

    drawn, agreed = [], []
    draw = engine_mod.draw_sampler_seed

    def recording_draw():
        drawn.append(draw())
        return drawn[-1]

    for mod_name, mod in list(sys.modules.items()):  # (``from baybe_amd.engine import draw_sampler_seed`` binds the name per module)
        if mod_name.startswith("baybe_amd") and getattr(mod, "draw_sampler_seed", None) is draw:
            monkeypatch.setattr(mod, "draw_sampler_seed", recording_draw)

    def agree(value):
        agreed.append("weights" if isinstance(value, np.ndarray) else value)
        return value

    space, exp, meas = _problem()
    kwargs, objective, batch = _paths(forest, linear)[name]
    rec = HipBotorchRecommender(**kwargs)
    n = len(exp)
    stub = _one_rank_shard(n, agree)
    calls = {
        "recommend": lambda pend: rec.recommend(batch, space, objective, meas, pending_experiments=pend),
        "values": lambda pend: rec.acquisition_values(exp.iloc[:5], space, objective, meas, pending_experiments=pend),
        "joint": lambda pend: rec.joint_acquisition_value(exp.iloc[[3, 9][:batch]], space, objective, meas, pending_experiments=pend),
    }
    out = {}
    for pending, sharded in ((False, False), (True, False), (False, True)):
        rec.shard = stub if sharded else None
        for call, fn in calls.items():
            del drawn[:], agreed[:]
            torch.manual_seed(17)
            np.random.seed(17)
            try:
                fn(exp.iloc[[7]] if pending else None)
                end = (int(torch.randint(0, 2**31 - 1, (1,)).item()), int(np.random.randint(0, 2**31 - 1)))
            except Exception as ex:  # noqa: BLE001
                if type(ex).__name__ not in REFUSALS:
                    raise
                end = type(ex).__name__
            out[(pending, sharded, call)] = (tuple(drawn), tuple(agreed), end)
    return out


# recorded on 962bac3: {path: {(pending, sharded, call): (seeds, agreed, (torch's next draw, numpy's next draw) or the refusal)}}
EXPECTED = {'single-mc': {(False, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
               (False, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
               (False, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
               (True, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
               (True, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
               (True, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
               (False, True, 'recommend'): ((576559,), (576559,), (1692828274, 1265576559)),
               (False, True, 'values'): ((576559,), (576559,), (1692828274, 1265576559)),
               (False, True, 'joint'): ((576559,), (576559,), (1692828274, 1265576559))},
 'single-analytic': {(False, False, 'recommend'): ((), (), (1164399056, 1265576559)),
                     (False, False, 'values'): ((), (), (1164399056, 1265576559)),
                     (False, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
                     (True, False, 'recommend'): ((), (), 'IncompatibleAcquisitionFunctionError'),
                     (True, False, 'values'): ((), (), 'IncompatibleAcquisitionFunctionError'),
                     (True, False, 'joint'): ((), (), 'IncompatibleAcquisitionFunctionError'),
                     (False, True, 'recommend'): ((), (), (1164399056, 1265576559)),
                     (False, True, 'values'): ((), (), (1164399056, 1265576559)),
                     (False, True, 'joint'): ((576559,), (576559,), (1692828274, 1265576559))},
 'transformed': {(False, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
                 (False, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
                 (False, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
                 (True, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
                 (True, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
                 (True, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
                 (False, True, 'recommend'): ((576559,), (576559,), (1692828274, 1265576559)),
                 (False, True, 'values'): ((576559,), (576559,), (1692828274, 1265576559)),
                 (False, True, 'joint'): ((576559,), (576559,), (1692828274, 1265576559))},
 'qNEI': {(False, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
          (False, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
          (False, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
          (True, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
          (True, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
          (True, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
          (False, True, 'recommend'): ((576559, 729585), (576559, 729585), (1741211303, 1265576559)),
          (False, True, 'values'): ((576559, 729585), (576559,), (1741211303, 1265576559)),
          (False, True, 'joint'): ((576559, 729585), (576559,), (1741211303, 1265576559))},
 'qLogNEI': {(False, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
             (False, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
             (False, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
             (True, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
             (True, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
             (True, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
             (False, True, 'recommend'): ((576559, 729585), (576559, 729585), (1741211303, 1265576559)),
             (False, True, 'values'): ((576559, 729585), (576559,), (1741211303, 1265576559)),
             (False, True, 'joint'): ((576559, 729585), (576559,), (1741211303, 1265576559))},
 'qLogNEHVI': {(False, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
               (False, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
               (False, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
               (True, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
               (True, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
               (True, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
               (False, True, 'recommend'): ((576559, 729585), (576559, 729585), (1741211303, 1265576559)),
               (False, True, 'values'): ((576559, 729585), (576559,), (1741211303, 1265576559)),
               (False, True, 'joint'): ((576559, 729585), (576559,), (1741211303, 1265576559))},
 'qNEHVI': {(False, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
            (False, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
            (False, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
            (True, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
            (True, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
            (True, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
            (False, True, 'recommend'): ((576559, 729585), (576559, 729585), (1741211303, 1265576559)),
            (False, True, 'values'): ((576559, 729585), (576559,), (1741211303, 1265576559)),
            (False, True, 'joint'): ((576559, 729585), (576559,), (1741211303, 1265576559))},
 'qLogNParEGO-drawn': {(False, False, 'recommend'): ((852751, 956742), (), (1167829095, 1265576559)),
                       (False, False, 'values'): ((852751, 956742), (), (1167829095, 1265576559)),
                       (False, False, 'joint'): ((852751, 956742), (), (1167829095, 1265576559)),
                       (True, False, 'recommend'): ((852751, 956742), (), (1167829095, 1265576559)),
                       (True, False, 'values'): ((852751, 956742), (), (1167829095, 1265576559)),
                       (True, False, 'joint'): ((852751, 956742), (), (1167829095, 1265576559)),
                       (False, True, 'recommend'): ((852751, 956742), ('weights', 852751, 956742), (1167829095, 1265576559)),
                       (False, True, 'values'): ((852751, 956742), ('weights', 852751), (1167829095, 1265576559)),
                       (False, True, 'joint'): ((852751, 956742), ('weights', 852751), (1167829095, 1265576559))},
 'qLogNParEGO-given': {(False, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
                       (False, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
                       (False, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
                       (True, False, 'recommend'): ((576559, 729585), (), (1741211303, 1265576559)),
                       (True, False, 'values'): ((576559, 729585), (), (1741211303, 1265576559)),
                       (True, False, 'joint'): ((576559, 729585), (), (1741211303, 1265576559)),
                       (False, True, 'recommend'): ((576559, 729585), (576559, 729585), (1741211303, 1265576559)),
                       (False, True, 'values'): ((576559, 729585), (576559,), (1741211303, 1265576559)),
                       (False, True, 'joint'): ((576559, 729585), (576559,), (1741211303, 1265576559))},
 'qLogEHVI': {(False, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
              (False, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
              (False, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
              (True, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
              (True, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
              (True, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
              (False, True, 'recommend'): ((), (), 'IncompatibilityError'),
              (False, True, 'values'): ((), (), 'IncompatibilityError'),
              (False, True, 'joint'): ((), (), 'IncompatibilityError')},
 'qNIPV': {(False, False, 'recommend'): ((576559,), (), (1692828274, 237259784)),
           (False, False, 'values'): ((576559,), (), (1692828274, 237259784)),
           (False, False, 'joint'): ((576559,), (), (1692828274, 237259784)),
           (True, False, 'recommend'): ((576559,), (), (1692828274, 237259784)),
           (True, False, 'values'): ((576559,), (), (1692828274, 237259784)),
           (True, False, 'joint'): ((576559,), (), (1692828274, 237259784)),
           (False, True, 'recommend'): ((), (), 'IncompatibilityError'),
           (False, True, 'values'): ((), (), 'IncompatibilityError'),
           (False, True, 'joint'): ((), (), 'IncompatibilityError')},
 'desirability-mc': {(False, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
                     (False, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
                     (False, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
                     (True, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
                     (True, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
                     (True, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
                     (False, True, 'recommend'): ((), (), 'IncompatibilityError'),
                     (False, True, 'values'): ((), (), 'IncompatibilityError'),
                     (False, True, 'joint'): ((), (), 'IncompatibilityError')},
 'desirability-analytic': {(False, False, 'recommend'): ((), (), (1164399056, 1265576559)),
                           (False, False, 'values'): ((), (), (1164399056, 1265576559)),
                           (False, False, 'joint'): ((), (), (1164399056, 1265576559)),
                           (True, False, 'recommend'): ((), (), 'IncompatibleAcquisitionFunctionError'),
                           (True, False, 'values'): ((), (), 'IncompatibleAcquisitionFunctionError'),
                           (True, False, 'joint'): ((), (), 'IncompatibleAcquisitionFunctionError'),
                           (False, True, 'recommend'): ((), (), 'IncompatibilityError'),
                           (False, True, 'values'): ((), (), 'IncompatibilityError'),
                           (False, True, 'joint'): ((), (), 'IncompatibilityError')},
 'forest-mc': {(False, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
               (False, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
               (False, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
               (True, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
               (True, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
               (True, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
               (False, True, 'recommend'): ((), (), 'IncompatibilityError'),
               (False, True, 'values'): ((), (), 'IncompatibilityError'),
               (False, True, 'joint'): ((), (), 'IncompatibilityError')},
 'linear-mc': {(False, False, 'recommend'): ((576559,), (), (1692828274, 1265576559)),
               (False, False, 'values'): ((576559,), (), (1692828274, 1265576559)),
               (False, False, 'joint'): ((576559,), (), (1692828274, 1265576559)),
               (True, False, 'recommend'): ((), (), 'IncompatibleSurrogateError'),
               (True, False, 'values'): ((), (), 'IncompatibleSurrogateError'),
               (True, False, 'joint'): ((), (), 'IncompatibleSurrogateError'),
               (False, True, 'recommend'): ((), (), 'IncompatibilityError'),
               (False, True, 'values'): ((), (), 'IncompatibilityError'),
               (False, True, 'joint'): ((), (), 'IncompatibilityError')}}


@pytest.mark.parametrize("name", PATH_NAMES)
def test_draw_order_is_the_parents(name, monkeypatch):
    got = _collect(name, monkeypatch)
    assert got == EXPECTED[name], {k: (v, EXPECTED[name].get(k)) for k, v in got.items() if v != EXPECTED[name].get(k)}
