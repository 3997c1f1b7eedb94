"""Desirability objectives with one model per target (``desirability="device"``), without a device.

  - ``baybe_amd.desirability.desirability_program`` against the reference's own ``DesirabilityObjective``: values of
    ``objective.to_botorch()`` on an [S, q, T] sample tensor, the weights / offset of ``to_botorch_posterior_transform()``, the
    program of a minimised target;
  - a real ``Campaign`` with the default ``DesirabilityObjective`` on the plug-in classes, the device doubled by the oracle
    (tests/_oracle_desirability.py): picks, acquisition values, one sampler seed per call, a partially measured row;
  - the refusals, each before any engine exists;
  - the guard of tests/test_desirability_gpu.py: every (case, scalariser, kind) it runs is one whose reference does not depend on
    who factored the covariances."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _desirability_cases as dc
import _objective_cases as oc
import _oracle_desirability as od
import _oracle_objective as oo
from _joint_cases import SCORE_ATOL
from _reference import reference_baybe
from baybe_amd.desirability import DesirabilityProgram, desirability_program
from baybe_amd.exceptions import IncompatibilityError

pytestmark = pytest.mark.filterwarnings("ignore")


# ---- descriptions against the reference's objective ---------------------------------------------------------------------------------
def _reference_targets(T):
    from baybe.targets import NumericalTarget as NT

    made = [
        NT.normalized_ramp("t0", (-1, 1.5)),
        NT.normalized_ramp("t1", (-2, 2), minimize=True),  # oriented: 1 - ramp
        NT.match_bell("t2", 0.4, 0.8),
        NT.normalized_sigmoid("t3", [(-1.0, 0.9), (1.5, 0.1)]),
        NT.normalized_ramp("t4", (-1, 1.5), descending=True),
        NT.match_triangular("t5", 0.5, cutoffs=(-1, 2)),
        NT.normalized_sigmoid("t6", [(-1.0, 0.1), (2.0, 0.9)], minimize=True),
        NT.normalized_ramp("t7", (0, 3)),
    ]
    return made[:T]


_WEIGHTS = {2: (2.0, 1.0), 3: (1.0, 2.5, 1.5), 8: (1.0, 2.0, 0.5, 1.5, 1.0, 3.0, 0.75, 1.25)}


@pytest.mark.parametrize("scalarizer", ["GEOM_MEAN", "MEAN"])
@pytest.mark.parametrize("T", [2, 3, 8])
def test_apply_equals_the_reference_objective(T, scalarizer):
    reference_baybe()
    from baybe.objectives import DesirabilityObjective

    objective = DesirabilityObjective(_reference_targets(T), weights=_WEIGHTS[T], scalarizer=scalarizer, require_normalization=False)
    prog = desirability_program(objective)
    assert isinstance(prog, DesirabilityProgram) and prog.n_targets == T and prog.scalarizer == scalarizer
    assert np.allclose(prog.normalized_weights, np.asarray(_WEIGHTS[T]) / np.sum(_WEIGHTS[T]), rtol=1e-15, atol=0)
    # the minimised ramp: its own affine map, the clamp, then ONE negation with the shift - not a second negation on top
    assert prog.programs[1].ops[-1] == ("AFFINE", (-1.0, 1.0)), prog.programs[1].ops
    samples = torch.from_numpy(np.random.default_rng(T).standard_normal((33, 4, T)) * 1.5)
    want = objective.to_botorch()(samples).numpy()
    got = prog.apply(samples.numpy())
    assert got.shape == want.shape == (33, 4)
    dev = float(np.abs(got - want).max())
    print(f"apply vs to_botorch [T={T}, {scalarizer}]: {dev:.3e}")
    assert dev <= 1e-12
    # the tests' own restatement agrees too
    assert np.abs(od.desirability(od.from_product(prog), samples.numpy()) - want).max() <= 1e-12
    assert prog.as_affine() is None  # (ramps and bells are not affine)


def test_minimised_identity_is_one_negation_plus_one():
    reference_baybe()
    from baybe.objectives import DesirabilityObjective
    from baybe.targets import NumericalTarget as NT

    objective = DesirabilityObjective([NT("a"), NT("b", minimize=True)], scalarizer="MEAN", require_normalization=False)
    prog = desirability_program(objective)
    assert prog.programs[0].ops == (("AFFINE", (1.0, 0.0)),)  # an identity is the one-operation program
    assert prog.programs[1].ops == (("AFFINE", (-1.0, 1.0)),)
    # a stand-in without ``_oriented_targets`` gets the same
    stand_in = dc.DesirabilityObjective([oc.affine_target("a", 1.0, 0.0), oc.affine_target("b", 1.0, 0.0, minimize=True)], scalarizer="MEAN")
    assert desirability_program(stand_in).programs[1].ops == (("AFFINE", (-1.0, 1.0)),)


def test_as_affine_equals_the_posterior_transform():
    reference_baybe()
    from baybe.objectives import DesirabilityObjective
    from baybe.targets import NumericalTarget as NT

    targets = [NT("a") * 2.5 + 1.0, NT("b", minimize=True), (NT("c") * -0.5 + 0.25).negate().negate()]
    targets[2] = NT("c", targets[2].transformation, minimize=True)
    objective = DesirabilityObjective(targets, weights=[1.0, 2.0, 0.5], scalarizer="MEAN", require_normalization=False)
    c, offset = desirability_program(objective).as_affine()
    try:
        pt = objective.to_botorch_posterior_transform()
        want_c, want_offset = pt.weights.numpy(), float(pt.offset)
    except ImportError:  # no BoTorch here: the same lines of the reference restated (objectives/desirability.py:294-319)
        oriented = [t.transformation if not t.minimize else t.transformation.negate() for t in targets]
        fs = [(getattr(tr, "factor", 1.0), getattr(tr, "shift", 0.0)) for tr in oriented]
        want_c = np.array([w * f for w, (f, _) in zip(objective.normalized_weights, fs)])
        want_offset = sum(w * s for w, (_, s) in zip(objective.normalized_weights, fs))
    assert np.allclose(c, want_c, rtol=1e-15, atol=0) and offset == pytest.approx(want_offset, rel=1e-15, abs=1e-16)
    geom = DesirabilityObjective([NT("a").clamp(0.1, 1), NT("b").clamp(0.1, 1)], scalarizer="GEOM_MEAN", require_normalization=False)
    assert desirability_program(geom).as_affine() is None


# ---- a real Campaign on the oracle double ------------------------------------------------------------------------------------------
@pytest.fixture()
def ref(monkeypatch):
    reference_baybe()
    eng = od.install(monkeypatch)
    from baybe_amd.plugin import make_baybe_classes

    S, C, R = make_baybe_classes()
    return S, C, R, eng


def _space3(levels=6):
    from baybe.parameters import NumericalDiscreteParameter
    from baybe.searchspace import SearchSpace

    vals = np.arange(levels) / (levels - 1)
    return SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])


def _measurements(space, n=16, seed=31):
    rng = np.random.default_rng(seed)
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), n, replace=False)].copy()
    X = meas[["x0", "x1", "x2"]].to_numpy(float)
    meas["gain"] = 100.0 * np.exp(-((X - 0.4) ** 2).sum(1)) + 0.5 * rng.standard_normal(n)
    meas["cost"] = 3.0 + 5.0 * X.sum(1) + 0.1 * rng.standard_normal(n)
    return meas


def _objective(**kw):
    from baybe.objectives import DesirabilityObjective
    from baybe.targets import NumericalTarget

    targets = [NumericalTarget.normalized_ramp("gain", cutoffs=(20, 100)),
               NumericalTarget.normalized_ramp("cost", cutoffs=(3, 18), minimize=True)]
    return DesirabilityObjective(targets, weights=[2.0, 1.0], **kw)


def _oracle_models(meas):
    """One oracle GP per target, each fitted on the rows where ITS target is measured."""
    from oracle import gp_oracle as go

    spec = go.GPSpec.baybe_default(3, np.zeros(3), np.ones(3))
    out = []
    for name in ("gain", "cost"):
        rows = meas[~meas[name].isna()]
        out.append(go.fit_gp(spec, rows[["x0", "x1", "x2"]].to_numpy(float), rows[name].to_numpy()))
    return out


def _seed_and_the_draw_after(seed_value):
    """(the next sampler seed, the draw after it): what the global generator hands out next, and after exactly one draw."""
    torch.manual_seed(seed_value)
    s = int(torch.randint(0, 1000000, (1,)).item())
    after = int(torch.randint(0, 1000000, (1,)).item())
    torch.manual_seed(seed_value)
    return s, after


def _one_seed_was_drawn(after):
    return int(torch.randint(0, 1000000, (1,)).item()) == after


def test_real_campaign_with_the_default_desirability_objective(ref):
    S, C, R, Eng = ref
    from baybe import Campaign

    space = _space3()
    exp = space.discrete.exp_rep
    meas = _measurements(space)
    meas.loc[meas.index[2], "cost"] = np.nan  # one row measured for 'gain' only
    objective = _objective()
    assert not objective.as_pre_transformation and not objective.is_multi_output
    des = od.from_product(desirability_program(objective))
    assert des.scalarizer == "GEOM_MEAN" and des.programs[1][-1] == ("AFFINE", (-1.0, 1.0))
    camp = Campaign(space, objective, R(desirability="device"))
    camp.add_measurements(meas)
    models = _oracle_models(meas)
    assert len(models[0].X_train) == 16 and len(models[1].X_train) == 15  # the row is used by the other target's model
    X_all = meas[["x0", "x1", "x2"]].to_numpy(float)
    bf = od.best_f(models, X_all, des)  # ... and in best_f: all 16 rows
    Xc = exp.to_numpy(float)

    seed, after = _seed_and_the_draw_after(99)
    got = camp.recommend(3)
    assert _one_seed_was_drawn(after)
    idx, _ = od.greedy(models, Xc, 3, seed, des, X_all)
    assert got.index.tolist() == exp.index[idx].tolist()
    engines = Eng.instances
    assert len(engines) == 2 and sorted(e.n for e in engines) == [15, 16]
    calls = [c[0] for c in engines[0].calls + engines[1].calls]
    assert calls.count("desirability_q1") == 1 and calls.count("desirability_pending") == 2
    rec = camp.recommender.recommender if hasattr(camp.recommender, "recommender") else camp.recommender
    assert rec._best_f == pytest.approx(bf, rel=1e-6, abs=1e-7)

    seed, after = _seed_and_the_draw_after(5)
    acq = camp.acquisition_values(exp.iloc[:40])
    assert _one_seed_was_drawn(after)
    want = od.model_scores(models, Xc[:40], None, des, "qLogEI", od.base_samples(512, 1, 2, seed), bf)
    assert np.allclose(acq.to_numpy(), want, rtol=1e-6, atol=1e-7)  # (two fits of the same data: the oracle's and the plug-in's)

    seed, after = _seed_and_the_draw_after(6)
    jv = camp.joint_acquisition_value(exp.iloc[[3, 40, 77]])
    assert _one_seed_was_drawn(after)
    rows = Xc[[3, 40, 77]]
    want = od.model_scores(models, rows[:1], rows[1:], des, "qLogEI", od.base_samples(512, 3, 2, seed), bf)[0]
    assert jv == pytest.approx(want, rel=1e-6, abs=1e-7)


def test_analytic_functions_take_the_affine_arithmetic_mean(ref):
    S, C, R, Eng = ref
    from baybe.objectives import DesirabilityObjective
    from baybe.targets import NumericalTarget as NT
    from oracle import gp_oracle as go

    space = _space3()
    exp = space.discrete.exp_rep
    meas = _measurements(space)
    objective = DesirabilityObjective([NT("gain") * 0.01, NT("cost", minimize=True)], weights=[2.0, 1.0], scalarizer="MEAN",
                                      require_normalization=False)
    prog = desirability_program(objective)
    c, offset = prog.as_affine()
    assert np.allclose(c, [2 / 3 * 0.01, -1 / 3]) and offset == 0.0  # minimised: negated, WITHOUT the + 1 of the MC objective
    models = _oracle_models(meas)
    Xc = exp.to_numpy(float)
    rec = R(acquisition_function="EI", desirability="device")
    acq = rec.acquisition_values(exp.iloc[:40], space, objective, meas)
    mv = [m.posterior(Xc[:40]) for m in models]
    mu = sum(ct * m for ct, (m, _) in zip(c, mv)) + offset
    var = sum(ct * ct * v for ct, (_, v) in zip(c, mv))
    best = od.best_f(models, meas[["x0", "x1", "x2"]].to_numpy(float), od.from_product(prog))  # the reference's own mix: the MC objective's incumbent
    want = go.analytic_acq("EI", mu, var, best, 1.0)
    assert np.allclose(acq.to_numpy(), want, rtol=1e-6, atol=1e-9)
    got = rec.recommend(1, space, objective, meas)
    mv = [m.posterior(Xc) for m in models]
    full = go.analytic_acq("EI", sum(ct * m for ct, (m, _) in zip(c, mv)) + offset, sum(ct * ct * v for ct, (_, v) in zip(c, mv)), best, 1.0)
    assert got.index.tolist() == [exp.index[int(np.argmax(full))]]


def test_refusals_come_before_any_engine(ref):
    S, C, R, Eng = ref
    from baybe.objectives import DesirabilityObjective
    from baybe.parameters import NumericalContinuousParameter, NumericalDiscreteParameter
    from baybe.searchspace import SearchSpace
    from baybe.targets import NumericalTarget as NT
    import baybe.exceptions
    import baybe_amd.exceptions

    Refused = (baybe.exceptions.IncompatibilityError, baybe_amd.exceptions.IncompatibilityError)
    space = _space3()
    meas = _measurements(space)
    objective = _objective()
    n_before = Eng.created
    # the default field value keeps today's refusal and both of its pinned phrases
    assert R().desirability == "refuse"
    with pytest.raises(Refused, match="as_pre_transformation=True") as info:
        R().recommend(2, space, objective, meas)
    assert "scalarise" in str(info.value) and "desirability='device'" in str(info.value)
    with pytest.raises(ValueError, match="desirability"):
        R(desirability="host")
    # nine targets
    nine = DesirabilityObjective([NT.normalized_ramp(f"t{i}", (0, 1)) for i in range(9)])
    meas9 = meas.assign(**{f"t{i}": np.linspace(0, 1, len(meas)) for i in range(9)})
    with pytest.raises(Refused, match="2 to 8 targets"):
        R(desirability="device").recommend(1, space, nine, meas9)
    # 17 points in one joint batch.  (BayBE's own ``recommend`` - in charge of the plug-in class - learns the batch size only after
    # the acquisition set-up; the stand-alone class checks it first, and the plug-in class still refuses, after its fit.)
    from baybe_amd.recommenders import HipBotorchRecommender

    with pytest.raises(Refused, match="exceeds 16"):
        HipBotorchRecommender(desirability="device").recommend(17, space, objective, meas)
    with pytest.raises(Refused, match="qLogExpectedImprovement"):
        R(acquisition_function="qLogNEI", desirability="device").recommend(1, space, objective, meas)
    with pytest.raises(Refused, match="requires a Gaussian distribution"):
        R(acquisition_function="EI", desirability="device").recommend(1, space, objective, meas)
    with pytest.raises(Refused, match="Row shards"):
        R(desirability="device", shard=SimpleNamespace(world=2, rank=0, N_total=216, start=0, stop=108)).recommend(1, space, objective, meas)
    hybrid = SearchSpace.from_product([NumericalDiscreteParameter("x0", (0.0, 0.5, 1.0)), NumericalDiscreteParameter("x1", (0.0, 1.0)),
                                       NumericalContinuousParameter("x2", (0.0, 1.0))])
    with pytest.raises(Refused, match="hybrid / continuous"):
        R(desirability="device").recommend(1, hybrid, objective, meas)
    assert Eng.created == n_before  # nothing was fitted
    with pytest.raises(Refused, match="exceeds 16"):
        R(desirability="device").recommend(17, space, objective, meas)


# ---- guard of the GPU cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jset", dc.JOINT_SETS, ids=[s.id for s in dc.JOINT_SETS])
def test_gpu_cases_do_not_depend_on_who_factored(jset):
    """For every (case, scalariser, kind) of tests/test_desirability_gpu.py: the score from LAPACK's factors (the oracle) and from
    the kernels' row-by-row factors agree to a quarter of the tolerance the device is held to, on every scored row - so a device
    miss is the device's.  The rows that do not factor are the labelled ones, target by target."""
    d = jset.build()
    Sig, means = d.sigmas()
    L_ref = np.stack([oo.lapack_factors(s) for s in Sig])
    L_row = np.stack([oo.rowwise_factors(s) for s in Sig])
    for t in range(jset.T):
        notpd = d.target_is_label(t, "notpd")
        assert np.array_equal(np.isnan(L_ref[t, :, 0, 0]), notpd) and np.array_equal(np.isnan(L_row[t, :, 0, 0]), notpd)
    assert d.scored.sum() >= min(jset.N, 40) or jset.N == 1, (jset.id, int(d.scored.sum()))
    assert jset.N == 1 or (d.notpd.sum() > d.target_is_label(0, "notpd").sum())  # rows that are not-PSD in SOME target only
    live = d.scored
    failures = []
    for scal in dc.SCALARIZERS:
        des = dc.description(jset.T, scal)
        bf = dc.case_best_f(des, d.mean)
        for kind in dc.MC_KINDS:
            a = od.scores_from_factors(kind, des, means, L_ref, d.z, bf, dc.BETA)[live]
            b = od.scores_from_factors(kind, des, means, L_row, d.z, bf, dc.BETA)[live]
            assert np.isfinite(a).all(), (jset.id, scal, kind)
            dev = float(np.abs(a - b).max())
            if dev > SCORE_ATOL / 4 or (kind != "qLogEI" and oc.mc_ratio(b, a) > 0.25):
                failures.append((scal, kind, dev, oc.mc_ratio(b, a)))
    assert not failures, failures
