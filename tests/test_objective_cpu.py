"""Target transformations as objective programs, without a device.

  - ``baybe_amd.objective.objective_program`` against the reference's own transformations for every constructor of
    ``NumericalTarget`` the path admits (values of the oriented transformation, and of ``objective.to_botorch()`` on an
    [S, q, 1] sample tensor), and its refusals;
  - a real ``Campaign`` with ``match_bell`` on the plug-in classes, the device doubled by the oracle
    (tests/_oracle_objective.py): picks, acquisition values, the analytic functions' affine rule;
  - the guard of tests/test_objective_gpu.py: every (case, program, kind) it runs is one whose reference does not depend on
    who factored the covariance."""

import numpy as np
import pytest
import torch

import _objective_cases as oc
import _oracle_objective as oo
from _joint_cases import SCORE_ATOL
from _reference import reference_baybe
from baybe_amd.exceptions import IncompatibilityError
from baybe_amd.objective import MAX_OPS, ObjectiveProgram, objective_program

pytestmark = pytest.mark.filterwarnings("ignore")


# ---- programs against the reference's transformations --------------------------------------------------------------------------
def _constructors(NT):
    return {
        "match_bell": lambda: NT.match_bell("y", 0.4, 0.8),
        "match_triangular": lambda: NT.match_triangular("y", 0.5, cutoffs=(-1, 2)),
        "match_triangular-mismatch": lambda: NT.match_triangular("y", 0.5, cutoffs=(-1, 2), mismatch_instead=True),
        "match_absolute": lambda: NT.match_absolute("y", 0.3),
        "match_quadratic": lambda: NT.match_quadratic("y", 0.3),
        "match_power3": lambda: NT.match_power("y", 0.3, 3),
        "normalized_ramp": lambda: NT.normalized_ramp("y", (-1, 1.5), descending=True),
        "normalized_sigmoid": lambda: NT.normalized_sigmoid("y", [(-1.0, 0.9), (1.5, 0.1)]),
        "clamp-log": lambda: NT("y").clamp(min=0.1).log(),
        "exp-clamp": lambda: NT("y").exp().clamp(max=5),
        "minimised-identity": lambda: NT("y", minimize=True),
        "affine-chain": lambda: (NT("y") * 2.5 + 1.0) * -0.5,
    }


CONSTRUCTORS = ("match_bell", "match_triangular", "match_triangular-mismatch", "match_absolute", "match_quadratic", "match_power3",
                "normalized_ramp", "normalized_sigmoid", "clamp-log", "exp-clamp", "minimised-identity", "affine-chain")
GRID = np.concatenate([np.linspace(-3.0, 3.0, 241), [0.1, 0.3, 0.4, 0.5, -1.0, 1.5, 2.0]])


@pytest.mark.parametrize("name", CONSTRUCTORS)
def test_program_equals_the_reference_transformation(name):
    reference_baybe()
    from baybe.targets import NumericalTarget

    t = _constructors(NumericalTarget)[name]()
    prog = objective_program(t)
    objective = t.to_objective()
    oriented = objective._oriented_targets[0].transformation
    want = oriented(torch.from_numpy(GRID)).numpy()
    if name == "minimised-identity":
        assert prog is None  # stays on the kernels' sign path
        assert np.array_equal(want, -GRID)
        return
    assert isinstance(prog, ObjectiveProgram) and 1 <= len(prog.ops) <= MAX_OPS
    got = prog.apply(GRID)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max() <= 1e-14, (name, prog.ops, np.abs(got[ok] - want[ok]).max())
    # the independent interpreter of the tests agrees as well (to rounding: it orders some products differently)
    assert np.abs(oo.apply_program(prog.ops, GRID)[ok] - want[ok]).max() <= 1e-14
    # ... and the MC objective BoTorch is handed: [S, q, 1] samples -> [S, q]
    samples = torch.from_numpy(np.random.default_rng(0).standard_normal((7, 3, 1)))
    mc = objective.to_botorch()(samples)
    mc = mc.numpy().reshape(7, 3)
    assert np.abs(prog.apply(samples.numpy()[..., 0]) - mc).max() <= 1e-14
    if name == "affine-chain":
        assert prog.ops == (("AFFINE", (-1.25, -0.5)),) and prog.as_affine() == (-1.25, -0.5)  # adjacent affines fold on the host


def test_listed_programs_are_what_the_constructors_give():
    """tests/_objective_cases.PROGRAMS (what the GPU module runs) against the reference's constructors."""
    reference_baybe()
    from baybe.targets import NumericalTarget as NT

    made = {
        "bell": NT.match_bell("y", 0.4, 0.8),
        "triangular-min": NT.match_triangular("y", 0.5, cutoffs=(-1, 2), mismatch_instead=True),
        "ramp": NT.normalized_ramp("y", (-1, 1.5), descending=True),
        "power3-min": NT.match_power("y", 0.3, 3),
        "clamp-log": NT("y").clamp(min=0.1).log(),
    }
    for name, t in made.items():
        got, want = objective_program(t).ops, oc.PROGRAMS[name]
        assert [o for o, _ in got] == [o for o, _ in want], (name, got)
        for (_, a), (_, b) in zip(got, want):
            assert np.allclose(a, b, rtol=1e-15, atol=0), (name, got)


def _stub(name, **attrs):
    return type(name, (), attrs)()


def _target(tr, minimize=False):
    return type("T", (), {"name": "y", "minimize": minimize, "transformation": tr})()


def test_refusals_name_the_class():
    affine = lambda a, b: _stub("AffineTransformation", factor=a, shift=b)  # noqa: E731
    for cls in ("CustomTransformation", "AdditiveTransformation", "MultiplicativeTransformation"):
        with pytest.raises(IncompatibilityError, match=cls):
            objective_program(_target(_stub(cls, transformations=(affine(1, 0), affine(2, 0)), function=abs)))
    with pytest.raises(IncompatibilityError, match="PowerTransformation"):
        objective_program(_target(_stub("PowerTransformation", exponent=2.5)))
    with pytest.raises(IncompatibilityError, match="BellTransformation"):  # parameters cannot be read
        objective_program(_target(_stub("BellTransformation")))
    with pytest.raises(IncompatibilityError, match="SomethingElseTransformation"):
        objective_program(_target(_stub("SomethingElseTransformation")))
    # nine operations that do not fold; eight are fine
    ops9 = tuple(x for _ in range(5) for x in (_stub("ExponentialTransformation"), _stub("LogarithmicTransformation")))[:9]
    with pytest.raises(IncompatibilityError, match="ChainedTransformation"):
        objective_program(_target(_stub("ChainedTransformation", transformations=ops9)))
    assert len(objective_program(_target(_stub("ChainedTransformation", transformations=ops9[:8]))).ops) == 8
    # a refused member inside a chain is found too
    with pytest.raises(IncompatibilityError, match="CustomTransformation"):
        objective_program(_target(_stub("ChainedTransformation", transformations=(affine(2, 0), _stub("CustomTransformation", function=abs)))))
    # identity, minimised or not: no program
    assert objective_program(_target(_stub("IdentityTransformation"))) is None
    assert objective_program(_target(_stub("IdentityTransformation"), minimize=True)) is None
    assert objective_program(type("T", (), {"name": "y", "minimize": True})()) is None


def test_reference_refusals_on_real_objects():
    reference_baybe()
    from baybe.targets import NumericalTarget as NT
    from baybe.transformations import CustomTransformation

    with pytest.raises(IncompatibilityError, match="CustomTransformation"):
        objective_program(NT("y", CustomTransformation(torch.abs)))
    with pytest.raises(IncompatibilityError, match="AdditiveTransformation"):
        objective_program(NT("y").log() + NT("y").exp())
    with pytest.raises(IncompatibilityError, match="PowerTransformation"):
        objective_program(NT("y").abs().power(2.5))


# ---- a real Campaign on the oracle double ----------------------------------------------------------------------------------------
@pytest.fixture()
def ref(monkeypatch):
    reference_baybe()
    eng = oo.install(monkeypatch)
    from baybe_amd.plugin import make_baybe_classes

    S, C, R = make_baybe_classes()
    return S, C, R, eng


def _space3(levels=8):
    from baybe.parameters import NumericalDiscreteParameter
    from baybe.searchspace import SearchSpace

    vals = np.arange(levels) / (levels - 1)
    return SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])


def _measurements(space, n=16, seed=0):
    rng = np.random.default_rng(seed)
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), n, replace=False)].copy()
    X = meas[["x0", "x1", "x2"]].to_numpy(float)
    meas["y"] = X.sum(1) - 0.8 + 0.3 * np.sin(3 * X[:, 0]) + 0.02 * rng.standard_normal(n)
    return meas


def _oracle_model(meas):
    from oracle import gp_oracle as go

    return go.fit_gp(go.GPSpec.baybe_default(3, np.zeros(3), np.ones(3)), meas[["x0", "x1", "x2"]].to_numpy(float), meas["y"].to_numpy())


def _next_sampler_seed(seed_value):
    torch.manual_seed(seed_value)
    s = int(torch.randint(0, 1000000, (1,)).item())
    torch.manual_seed(seed_value)
    return s


def test_real_campaign_with_match_bell(ref):
    S, C, R, Eng = ref
    from baybe import Campaign
    from baybe.targets import NumericalTarget

    space = _space3()
    exp = space.discrete.exp_rep
    meas = _measurements(space)
    target = NumericalTarget.match_bell("y", 0.4, 0.3)
    ops = objective_program(target).ops
    camp = Campaign(space, target.to_objective(), R())
    camp.add_measurements(meas)
    model = _oracle_model(meas)
    seed = _next_sampler_seed(99)
    got = camp.recommend(3)
    idx, _ = oo.greedy(model, exp.to_numpy(float), 3, seed, ops)
    assert got.index.tolist() == exp.index[idx].tolist()
    assert any(c[0] == "mc_acq_obj_pending" for e in Eng.instances for c in e.calls)  # the picks went through the program
    seed = _next_sampler_seed(5)
    acq = camp.acquisition_values(exp.iloc[:40])
    from oracle import gp_oracle as go

    z = go.sobol_normal_base_samples(512, 1, seed)
    want = oo.model_scores(model, exp.iloc[:40].to_numpy(float), None, ops, "qLogEI", z, oo.best_f(model, ops))
    assert np.allclose(acq.to_numpy(), want, rtol=1e-6, atol=1e-7)  # (two fits of the same data: the oracle's and the plug-in's)
    seed = _next_sampler_seed(6)
    jv = camp.joint_acquisition_value(exp.iloc[[3, 40, 77]])
    z = go.sobol_normal_base_samples(512, 3, seed)
    rows = exp.iloc[[3, 40, 77]].to_numpy(float)
    want = oo.model_scores(model, rows[:1], rows[1:], ops, "qLogEI", z, oo.best_f(model, ops))[0]
    assert jv == pytest.approx(want, rel=1e-6, abs=1e-7)
    # more than 16 points in one joint batch: refused with the batch-size wording, before anything is scored
    with pytest.raises(IncompatibilityError, match="exceeds 16"):
        R().recommend(17, space, target.to_objective(), meas)


def test_analytic_functions_take_affine_programs_only(ref):
    S, C, R, Eng = ref
    from baybe.targets import NumericalTarget
    from oracle import gp_oracle as go

    space = _space3()
    exp = space.discrete.exp_rep
    meas = _measurements(space)
    model = _oracle_model(meas)
    a, b = -2.0, 0.5
    target = NumericalTarget("y") * a + b
    assert objective_program(target).as_affine() == (a, b)
    rec = R(acquisition_function="EI")
    acq = rec.acquisition_values(exp.iloc[:40], space, target.to_objective(), meas)
    mu, var = model.posterior(exp.iloc[:40].to_numpy(float))
    best = float((a * model.posterior(model.X_train)[0] + b).max())
    want = go.analytic_acq("EI", a * mu + b, a * a * var, best, 1.0)
    assert np.allclose(acq.to_numpy(), want, rtol=1e-6, atol=1e-9)
    got = rec.recommend(1, space, target.to_objective(), meas)
    full = go.analytic_acq("EI", *(lambda m, v: (a * m + b, a * a * v))(*model.posterior(exp.to_numpy(float))), best, 1.0)
    assert got.index.tolist() == [exp.index[int(np.argmax(full))]]
    with pytest.raises(IncompatibilityError, match="requires a Gaussian distribution"):
        rec.recommend(1, space, NumericalTarget.match_bell("y", 0.4, 0.3).to_objective(), meas)


def test_transformed_targets_stay_refused_where_the_issue_leaves_them(ref):
    S, C, R, Eng = ref
    from baybe.objectives import ParetoObjective
    from baybe.targets import NumericalTarget

    space = _space3()
    meas = _measurements(space)
    meas["z"] = -meas["y"]
    bell = NumericalTarget.match_bell("y", 0.4, 0.3)
    n_before = Eng.created
    with pytest.raises(IncompatibilityError, match="BellTransformation"):
        R(acquisition_function="qLogNEI").recommend(1, space, bell.to_objective(), meas)
    with pytest.raises(IncompatibilityError, match="BellTransformation"):
        R().recommend(1, space, ParetoObjective([bell, NumericalTarget("z")]), meas)
    assert Eng.created == n_before  # nothing was fitted


# ---- guard of the GPU cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.JOINT_CASES, ids=[c.id for c in oc.JOINT_CASES])
def test_gpu_cases_do_not_depend_on_who_factored(case):
    """For every (case, program, kind) of tests/test_objective_gpu.py: the score from LAPACK's factor (the oracle) and from the
    kernels' row-by-row factor agree to a quarter of the tolerance the device is held to, on every scored row - so a device
    miss is the device's.  The rows that score NaN / -inf are the labelled ones."""
    d = case.build()
    Sig, means = oo.case_sigma(d)
    L_ref, L_row = oo.lapack_factors(Sig), oo.rowwise_factors(Sig)
    assert np.array_equal(np.isnan(L_ref[:, 0, 0]), d.is_label("notpd")) and np.array_equal(np.isnan(L_row[:, 0, 0]), d.is_label("notpd"))
    live = d.scored
    failures = []
    for pname, ops in oc.PROGRAMS.items():
        bf = oc.case_best_f(ops, d.mean)
        for kind in oc.MC_KINDS:
            a = oo.scores_from_factors(kind, ops, means, L_ref, d.z, bf, oc.BETA)[live]
            b = oo.scores_from_factors(kind, ops, means, L_row, d.z, bf, oc.BETA)[live]
            assert np.isfinite(a).all(), (case.id, pname, kind)
            dev = float(np.abs(a - b).max())
            bound = SCORE_ATOL / 4
            if dev > bound or (kind != "qLogEI" and oc.mc_ratio(b, a) > 0.25):
                failures.append((pname, kind, dev, oc.mc_ratio(b, a)))
    assert not failures, failures
