"""qNIPV without a GPU: the oracle's two forms against each other and the fixtures of tests/test_nipv_gpu.py (tests/_nipv_cases.py), the
integration points against the reference's own ``sample_numerical_df``, the acquisition class against the reference's, the conversion
and the recommender's refusals - every one before anything is fitted."""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import _nipv_cases as nc
import _oracle_fps as oracle_fps
import _oracle_nipv as on
from _baybe_shim import NumericalTarget, SearchSpace, SingleTargetObjective
from _reference import reference_baybe
from baybe_amd import acquisition as A
from baybe_amd import sampling
from baybe_amd.exceptions import IncompatibilityError, IncompatibleAcquisitionFunctionError

ALL_CASES = nc.CASES + [nc.ASSEMBLY_CASE, nc.REFACTOR_CASE] + nc.GREEDY_CASES


# ---- the oracle and the fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_oracle_forms_agree_and_the_fixture_is_well_conditioned(case):
    """Form (a) (Cholesky of the conditioned system) and form (b) (Schur complement on posterior covariances) agree within the bound at
    c = 1 on every row; cond(K + s2 I) <= 1e4, standardised noise >= 0.01, no jitter."""
    c = case.build()
    a, s = (on.direct(c.om, c.X, c.B, c.P), on.schur(c.om, c.X, c.B, c.P)) if case in nc.GREEDY_CASES else case.reference()
    ratio = np.abs(a.gain - s.gain) / s.tol
    print(f"{case.id}: max |a - b| / tol(c = 1) = {ratio.max():.4f}, cond = {on.condition_number(c.om):.0f}")
    assert ratio.max() <= 1.0, (case.id, ratio.max())
    assert np.abs(a.value - s.value).max() <= s.tol.max() / case.M + 8 * on.EPS * abs(a.v_b)
    assert abs(a.v_b - s.v_b) <= 64 * on.EPS * abs(a.v_b) * on.condition_number(c.om) ** 0.5
    assert np.all(a.gain > 0) and np.all(s.tol > 0) and np.all(s.tol < 1e-6 * s.gain)
    assert on.condition_number(c.om) <= nc.MAX_COND and c.noise >= 0.01 and c.om.jitter == 0.0
    assert np.allclose(a.den, s.den, rtol=1e-9)


def test_shapes_cover_every_axis_value_and_the_edges_of_the_column_block():
    ns, Ns, bs, ds, kernels, Ms = (set(getattr(c, k) for c in nc.CASES) for k in ("n", "N", "b", "d", "kernel", "M"))
    assert ns == {1, 16, 17, 130, 512} and Ns == {1, 17, 257} and bs == {0, 1, 15} and ds == {1, 20}
    assert kernels == {"matern12", "matern32", "matern52", "rbf"}
    B = nc.COLBLOCK
    assert {1, B - 1, B, B + 1} <= Ms and any(m > 2 * B and m % B for m in Ms)
    corner = max(nc.CASES, key=lambda c: c.M)
    assert (corner.n, corner.b) == (512, 15) and -(-corner.M // nc.SLICE) >= 3  # three slices of the second grid dimension
    c = corner.build()
    assert np.array_equal(c.X[0], c.P[0]) and np.array_equal(c.X[1], c.Xt[0]) and np.array_equal(c.X[2], c.B[0])
    assert np.array_equal(c.X[3], c.X[-1]) and c.alive[4] == 0 and np.array_equal(c.P[-1], c.P[1])


def test_a_candidate_on_a_training_row_has_a_small_gain_with_an_absolute_bound():
    """gain near 0 is where a relative bound would fail: the bound is absolute and stays far below the gains it has to tell apart."""
    for case in nc.CASES:
        if case.N < 17:
            continue
        a, s = case.reference()
        assert a.gain[1] < np.median(a.gain), case.id  # (the row that IS training row 0)
        assert s.tol[1] > 0 and np.isfinite(s.tol[1])


def test_greedy_fixtures_are_decidable_by_the_oracle_alone():
    """At most 1 greedy step in 10 may be left out of the pick comparison (top-two gap below the sum of both rows' bounds): the seeds
    are chosen so that the oracle meets that at the shipped constant and at the largest one the issue admits."""
    for c_bound in (nc.C_BOUND, nc.C_CAP):
        steps = [st for case in nc.GREEDY_CASES for st in nc.greedy_reference(case.id)]
        left_out = sum(not nc.decidable(st, c_bound) for st in steps)
        assert len(steps) == nc.GREEDY_Q * len(nc.GREEDY_CASES) and left_out <= nc.MAX_LEFT_OUT * len(steps), (c_bound, left_out)
    assert nc.C_BOUND <= nc.C_CAP and np.log2(nc.C_BOUND) == int(np.log2(nc.C_BOUND))
    for case in nc.GREEDY_CASES:
        assert case.b == 2 and len({st.index for st in nc.greedy_reference(case.id)}) == nc.GREEDY_Q


# ---- integration points -------------------------------------------------------------------------------------------------------------
def _space(rows=30, seed=4):
    rng = np.random.default_rng(seed)
    return SearchSpace.from_dataframe(pd.DataFrame(rng.random((rows, 3)), columns=["x0", "x1", "x2"]))


@pytest.fixture()
def fps_double(monkeypatch):
    """The oracle-backed stand-in for the device surface of farthest point sampling (tests/test_fps_cpu.py)."""
    monkeypatch.setattr(sampling, "_points_factory", oracle_fps.OraclePoints)
    oracle_fps.OraclePoints.instances.clear()


POINT_SETTINGS = [dict(sampling_n_points=1), dict(sampling_n_points=7), dict(sampling_fraction=0.2), dict(), dict(sampling_n_points=70),
                  dict(sampling_n_points=60)]


@pytest.mark.parametrize("method", ["Random", "FPS"])
@pytest.mark.parametrize("setting", POINT_SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "default")
def test_integration_points_against_the_references_sample_numerical_df(setting, method, fps_double):
    """Identical ilocs: Random under the same ``np.random.seed`` (and the same state of the global generator afterwards), FPS on points
    without distance ties; n above the row count repeats the whole frame and samples the remainder."""
    from baybe_amd.nipv import integration_points

    reference_baybe()
    from baybe.acquisition.acqfs import qNegIntegratedPosteriorVariance as RefNIPV
    from baybe.utils.sampling_algorithms import DiscreteSamplingMethod, sample_numerical_df

    space = _space()
    comp = space.discrete.comp_rep
    ref_acqf = RefNIPV(sampling_method=method, **setting)
    n = ref_acqf.sampling_n_points or int(np.ceil(ref_acqf.sampling_fraction * len(comp)))
    np.random.seed(11)
    want = sample_numerical_df(comp, n, method=DiscreteSamplingMethod(method))
    state_want = np.random.get_state()[1].copy()
    np.random.seed(11)
    got = integration_points(A.qNIPV(sampling_method=method, **setting), space)
    state_got = np.random.get_state()[1].copy()
    assert len(got) == n and got.index.tolist() == want.index.tolist()
    assert np.array_equal(got.to_numpy(), want.to_numpy())
    if method == "Random":
        assert np.array_equal(state_got, state_want)
    # the reference's own object (its enum member as the method) gives the same rows
    np.random.seed(11)
    assert integration_points(A.convert_acqf(ref_acqf, nipv="device"), space).index.tolist() == want.index.tolist()


def test_integration_points_use_all_rows_not_the_candidates_left():
    from baybe_amd.nipv import integration_points

    space = _space()
    keep = np.ones(30, dtype=bool)
    keep[:20] = False
    filtered = space.filtered(keep)
    got = integration_points(A.qNIPV(), filtered)
    assert len(got) == 30 and got.index.tolist() == list(range(30))


# ---- the acquisition class ----------------------------------------------------------------------------------------------------------
def test_class_attributes_and_alias():
    cls = A.qNegIntegratedPosteriorVariance
    assert A.qNIPV is cls and cls.abbreviation == "qNIPV" and cls.kind == "qNIPV"
    assert cls.supports_batching and cls.supports_pending_experiments and not cls.supports_multi_output and cls.is_mc and not cls.is_analytic
    d = cls()
    assert (d.sampling_n_points, d.sampling_fraction, d.sampling_method) == (None, 1.0, "Random")
    p = cls(sampling_n_points=5, sampling_method="FPS")
    assert (p.sampling_n_points, p.sampling_fraction, p.sampling_method) == (5, None, "FPS")


BAD_SETTINGS = [dict(sampling_n_points=3, sampling_fraction=0.5), dict(sampling_n_points=0), dict(sampling_n_points=2.0),
                dict(sampling_fraction=0.0), dict(sampling_fraction=1.5), dict(sampling_method="Sobol")]


@pytest.mark.parametrize("setting", BAD_SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_validators_and_texts_against_the_references_class(setting):
    reference_baybe()
    from baybe.acquisition.acqfs import qNegIntegratedPosteriorVariance as RefNIPV

    with pytest.raises((ValueError, TypeError)) as ref:
        RefNIPV(**setting)
    with pytest.raises(type(ref.value)) as ours:
        A.qNIPV(**setting)
    if "sampling_method" not in setting:  # (the enum's own message names the enum class)
        assert str(ours.value) == str(ref.value)
    if len(setting) == 2:
        assert "cannot be specified at the same time" in str(ours.value)
    for good in (dict(), dict(sampling_n_points=4), dict(sampling_fraction=0.25, sampling_method="FPS")):
        r, o = RefNIPV(**good), A.qNIPV(**good)
        assert (r.sampling_n_points, r.sampling_fraction, r.sampling_method.value) == (o.sampling_n_points, o.sampling_fraction, o.sampling_method)
    assert RefNIPV.abbreviation == A.qNIPV.abbreviation
    for flag in ("supports_batching", "supports_pending_experiments", "supports_multi_output", "is_mc", "is_analytic"):
        if hasattr(RefNIPV, flag):
            assert bool(getattr(RefNIPV, flag)) == bool(getattr(A.qNIPV, flag)), flag


# ---- conversion ------------------------------------------------------------------------------------------------------------------------
def test_convert_acqf_refuses_by_default_and_converts_on_request():
    standin = type("qNegIntegratedPosteriorVariance", (), {"sampling_n_points": 9, "sampling_fraction": None, "sampling_method": "FPS"})()
    for spelling in ("qNIPV", "qNegIntegratedPosteriorVariance", standin, A.qNIPV()):
        for kw in (dict(), dict(nipv="refuse"), dict(ehvi="device")):
            with pytest.raises(IncompatibleAcquisitionFunctionError, match="not available on this path") as info:
                A.convert_acqf(spelling, **kw)
            assert "nipv='device'" in str(info.value)
    for spelling in ("qNIPV", "qNegIntegratedPosteriorVariance"):
        got = A.convert_acqf(spelling, nipv="device")  # a TypeError without the feature
        assert type(got) is A.qNIPV and (got.sampling_n_points, got.sampling_fraction, got.sampling_method) == (None, 1.0, "Random")
    got = A.convert_acqf(standin, nipv="device")
    assert type(got) is A.qNIPV and (got.sampling_n_points, got.sampling_fraction, got.sampling_method) == (9, None, "FPS")
    own = A.qNIPV(sampling_fraction=0.5)
    assert A.convert_acqf(own, nipv="device") is own
    # the setting opens nothing else, and nothing else opens it
    for name in ("qEHVI", "qLogEHVI", "qKG", "qTS"):
        with pytest.raises(IncompatibleAcquisitionFunctionError, match="not available on this path"):
            A.convert_acqf(name, nipv="device")
    assert type(A.convert_acqf("qEHVI", ehvi="device", nipv="device")) is A.qEHVI
    for nipv in ("refuse", "device"):
        assert type(A.convert_acqf("qLogEI", nipv=nipv)) is A.qLogEI and type(A.convert_acqf("qLogNEHVI", nipv=nipv)) is A.qLogNEHVI


def test_convert_acqf_takes_the_references_own_object():
    reference_baybe()
    from baybe.acquisition.acqfs import qNegIntegratedPosteriorVariance as RefNIPV

    got = A.convert_acqf(RefNIPV(sampling_n_points=12, sampling_method="FPS"), nipv="device")
    assert type(got) is A.qNIPV and (got.sampling_n_points, got.sampling_fraction, got.sampling_method) == (12, None, "FPS")
    with pytest.raises(IncompatibleAcquisitionFunctionError, match="nipv='device'"):
        A.convert_acqf(RefNIPV())


def test_recommender_field_and_plugin_fields():
    import attrs

    from baybe_amd import _lib
    from baybe_amd.recommenders import HipBotorchRecommender as R
    from baybe_amd.recommenders import recommender_fields

    assert R().nipv == "refuse" and R(nipv="device").nipv == "device"
    with pytest.raises(ValueError, match="nipv"):
        R(nipv="host")
    with pytest.raises(TypeError):
        R(None, "device")  # keyword-only
    with pytest.raises(IncompatibleAcquisitionFunctionError, match="nipv='device'"):
        R(acquisition_function="qNIPV")
    assert type(R(nipv="device", acquisition_function="qNIPV").acquisition_function) is A.qNIPV  # a TypeError without the feature
    assert type(R(acquisition_function=A.qNIPV(sampling_n_points=3), nipv="device").acquisition_function) is A.qNIPV  # whatever the order
    with pytest.raises(IncompatibleAcquisitionFunctionError):
        R(ehvi="device", acquisition_function="qNIPV")
    f = recommender_fields(with_base_fields=False)
    cls = attrs.make_class("P", {"nipv": f["nipv"]})
    assert cls().nipv == "refuse" and cls(nipv="device").nipv == "device"
    assert {"bbh_nipv_set_points", "bbh_nipv_gain", "bbh_last_nipv_form"} <= set(_lib.SIGNATURES)
    import copy

    rec = R(nipv="device", acquisition_function="qNIPV")
    rec._scorer = object()
    assert copy.deepcopy(rec)._scorer is None and copy.deepcopy(rec).nipv == "device"  # per-call state is dropped on copy


# ---- refusals, before anything is fitted -----------------------------------------------------------------------------------------------
class _UntouchableSurrogate:
    """Stands in for the GP surrogate: its settings can be read, any use is an error."""

    kernel = "matern52"
    kernel_or_factory = None
    preset = "BAYBE"
    use_outputscale = False
    supports_multi_output = False

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def fit(self, *a, **k):
        raise AssertionError("the surrogate was fitted")

    def replicate(self):
        return self

    @property
    def engine(self):
        raise AssertionError("the engine was used")


def _stub(name, **fields):
    return type(name, (), fields)()


def _problem(n=8, task=False):
    space = _space()
    if task:
        # (a subclass of its own: the shim's class stays as it is)
        space = type("TaskSpace", (type(space),), {"task_idx": property(lambda self: 0)})(space.discrete)
    exp = space.discrete.exp_rep
    meas = exp.iloc[np.arange(n) % len(exp)].copy()
    meas["t"] = np.linspace(0.0, 1.0, n)
    return space, meas, SingleTargetObjective(NumericalTarget("t"))


def _refusal_cases():
    from baybe_amd.forest import HipRandomForestSurrogate
    from baybe_amd.kernels import MaternKernel, ProductKernel, RBFKernel
    from baybe_amd.linear import HipBayesianLinearSurrogate

    bent = NumericalTarget("t")
    bent.transformation = _stub("AffineTransformation", factor=2.0, shift=1.0)
    two = SimpleNamespace(targets=(NumericalTarget("t"), NumericalTarget("u")), is_multi_output=False)
    I = IncompatibilityError
    return {
        "target transformation": (I, "currently does not support any target transformations", dict(objective=SingleTargetObjective(bent))),
        "desirability on the device": (I, "DesirabilityObjective", dict(objective=two, rec=dict(desirability="device"))),
        "hybrid space": (I, "hybrid / continuous", dict(hybrid=True)),
        "row shards": (I, "Row shards", dict(rec=dict(shard=SimpleNamespace(world=2, rank=0, agree=lambda v: v)))),
        "forest surrogate": (I, "HipRandomForestSurrogate", dict(surrogate_object=HipRandomForestSurrogate)),
        "linear surrogate": (I, "HipBayesianLinearSurrogate", dict(surrogate_object=HipBayesianLinearSurrogate)),
        "RFF kernel": (I, "the kernel 'rff'", dict(surrogate=dict(kernel="rff"))),
        "task parameter": (I, "task parameters", dict(task=True)),
        "composite kernel": (I, "composite kernel", dict(surrogate=dict(kernel=ProductKernel([MaternKernel(), RBFKernel()])))),
        "kernel factory": (I, "kernel factory", dict(surrogate=dict(kernel_or_factory=lambda *a, **k: None))),
        "more than 512 training points": (I, "512 training points", dict(n=513)),
        "pending + batch_size > 15": (I, "limit of 15", dict(batch=8, pending=8)),
    }


@pytest.mark.parametrize("case", list(_refusal_cases()))
def test_refusals_come_before_anything_is_fitted(case, monkeypatch):
    from baybe_amd import engine as engine_mod
    from baybe_amd.recommenders import HipBotorchRecommender as R

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the refusal")

    monkeypatch.setattr(engine_mod, "HipGP", NoEngine)
    error, text, how = _refusal_cases()[case]
    space, meas, objective = _problem(how.get("n", 8), how.get("task", False))
    if how.get("hybrid"):
        space = type(space)(space.discrete)
        space.continuous = SimpleNamespace(is_empty=False, comp_rep_bounds=pd.DataFrame({"c": [0.0, 1.0]}))
    surrogate = how["surrogate_object"]() if "surrogate_object" in how else _UntouchableSurrogate(**how.get("surrogate", {}))
    rec = R(nipv="device", acquisition_function="qNIPV", surrogate_model=surrogate, **how.get("rec", {}))
    pend = space.discrete.exp_rep.iloc[: how["pending"]] if "pending" in how else None
    with pytest.raises(error, match=text) as info:
        rec.recommend(how.get("batch", 1), space, how.get("objective", objective), meas, pending_experiments=pend)
    assert any(w in str(info.value) for w in ("Use", "use", "Recommend", "score the candidates"))  # says what to do instead
    if "objective" not in how and "batch" not in how:  # the read-back entry points refuse the same way (they have no batch size)
        with pytest.raises(error, match=text):
            rec.acquisition_values(space.discrete.exp_rep.iloc[:3], space, objective, meas, pending_experiments=pend)


def test_a_pareto_objective_falls_to_the_single_output_check():
    from _baybe_shim import ParetoObjective
    from baybe_amd.recommenders import HipBotorchRecommender as R

    space, meas, _ = _problem()
    meas["u"] = meas["t"] ** 2
    rec = R(nipv="device", acquisition_function="qNIPV", surrogate_model=_UntouchableSurrogate())
    with pytest.raises(IncompatibleAcquisitionFunctionError, match="single-output acquisition function"):
        rec.recommend(1, space, ParetoObjective([NumericalTarget("t"), NumericalTarget("u")]), meas)


@pytest.mark.parametrize("minimize", [False, True])
def test_what_is_covered_reaches_the_fit(minimize):
    """Nothing is refused for a MIN or MAX target, each of the four kernels, 15 conditioned points: the fit is the next thing."""
    from baybe_amd.recommenders import HipBotorchRecommender as R

    space, meas, _ = _problem(n=512)
    objective = SingleTargetObjective(NumericalTarget("t", minimize=minimize))
    for kernel in ("matern12", "matern32", "matern52", "rbf"):
        rec = R(nipv="device", acquisition_function=A.qNIPV(sampling_n_points=5), surrogate_model=_UntouchableSurrogate(kernel=kernel))
        with pytest.raises(AssertionError, match="the surrogate was fitted"):
            rec.recommend(8, space, objective, meas, pending_experiments=space.discrete.exp_rep.iloc[:7])


def test_the_baybe_typed_recommender_takes_the_references_own_object():
    """``plugin.make_baybe_classes()``: BayBE's own ``acquisition_function`` field keeps the reference's ``qNIPV(...)`` object; the
    ``nipv`` setting decides at use whether it converts (copying its three fields) or is refused."""
    reference_baybe()
    from baybe.acquisition.acqfs import qNegIntegratedPosteriorVariance as RefNIPV
    from baybe.recommenders.pure.bayesian.base import BayesianRecommender
    from baybe_amd import plugin

    _, _, Rec = plugin.make_baybe_classes()
    ref = RefNIPV(sampling_n_points=12, sampling_method="FPS")
    rec = Rec(nipv="device", acquisition_function=ref)
    assert isinstance(rec, BayesianRecommender) and rec.nipv == "device" and rec.acquisition_function is ref
    got = rec._get_acquisition_function(SingleTargetObjective(NumericalTarget("t")))
    assert type(got) is A.qNIPV and (got.sampling_n_points, got.sampling_fraction, got.sampling_method) == (12, None, "FPS")
    assert Rec(acquisition_function=ref).nipv == "refuse"
    with pytest.raises(IncompatibleAcquisitionFunctionError, match="nipv='device'"):
        Rec(acquisition_function=ref)._get_acquisition_function(SingleTargetObjective(NumericalTarget("t")))
