"""qEHVI / qLogEHVI without a GPU: the numpy oracle of tests/_oracle_ehvi.py against the exact hypervolume difference and against
``oracle/nehvi_oracle.py`` at q' = 1, the host set-up of ``baybe_amd/ehvi.py`` (``make_partitioning``, the alpha rule), the opt-in
conversion of ``baybe_amd/acquisition.py``, every refusal of the recommender before anything is fitted, and the guards of the
inputs tests/test_ehvi_gpu.py runs on the device."""

from types import SimpleNamespace

import numpy as np
import pytest

import _ehvi_cases as ec
import _objective_cases as oc
import _oracle_ehvi as oe
import _oracle_objective as oo
from _joint_cases import SCORE_ATOL
from baybe_amd import acquisition as A
from baybe_amd.exceptions import IncompatibilityError, IncompatibleAcquisitionFunctionError
from oracle import nehvi_oracle as no


# ---- the oracle itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ec.TARGET_COUNTS)
def test_plain_oracle_equals_the_exact_hypervolume_difference(m):
    """Inclusion-exclusion over the cells = hypervolume(front + batch) - hypervolume(front), for q' = 1, 2, 3, 4, 6 points with
    correlations 0, 0.9, 0.9999 and 1 between them, 7 front points, 16 samples.  Both sides carry the rounding of a hypervolume of
    the size of hypervolume(front + batch), so that is what 1e-12 is relative to (observed: 4e-15)."""
    P, ref = ec.front(m, 7), np.full(m, ec.REF)
    lo, up = ec.cells(m, 7)
    rng = np.random.default_rng(m)
    worst = 0.0
    for q in (1, 2, 3, 4, 6):
        for rho in (0.0, 0.9, 0.9999, 1.0):
            shared = rng.standard_normal((16, 1, m))
            Y = 0.3 + 1.2 * (rho * shared + np.sqrt(1.0 - rho * rho) * rng.standard_normal((16, q, m)))
            got = oe.qehvi_samples(Y, lo, up)
            for s in range(16):
                total = no.hypervolume(np.vstack([P, Y[s]]), ref)
                want = total - no.hypervolume(P, ref)
                worst = max(worst, abs(got[s] - want) / total)
    print(f"m = {m}: worst relative deviation {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("m", ec.TARGET_COUNTS)
@pytest.mark.parametrize("k", ec.FRONT_SIZES)
def test_log_oracle_at_q1_is_the_nehvi_estimator_with_one_cell_list(m, k):
    mean, var, z, alive = ec.q1_inputs(257, 33, m)
    lo, up = ec.cells(m, k)
    got = oe.q1_scores(True, mean, var, z, lo, up)
    from oracle import gp_oracle as go

    sd = np.stack([go._safe_sqrt_var(v) for v in var])
    for i in (0, 3, 5, 77, 256):
        f = mean[:, i][None, :] + sd[:, i][None, :] * z  # [S, m]
        want = no.logmeanexp_with_neginf(np.array([no.log_hvi_smoothed(f[s], lo, up) for s in range(len(z))]))
        assert got[i] == pytest.approx(want, rel=0, abs=1e-12)
    plain = oe.q1_scores(False, mean, var, z, lo, up)
    f = mean[:, 77][None, :] + sd[:, 77][None, :] * z
    assert plain[77] == pytest.approx(np.mean([no.hvi_from_cells(f[s], lo, up) for s in range(len(z))]), rel=1e-13)


def test_log_oracle_is_finite_on_every_live_fixture_row():
    for N, S in ec.Q1_SHAPES:
        for m in ec.TARGET_COUNTS:
            mean, var, z, alive = ec.q1_inputs(N, S, m)
            for k in ec.FRONT_SIZES:
                for log in (True, False):
                    assert np.isfinite(oe.q1_scores(log, mean, var, z, *ec.cells(m, k))).all(), (N, S, m, k, log)
    assert [len(ec.cells(m, 0)[0]) for m in ec.TARGET_COUNTS] == [1, 1, 1] and np.isinf(ec.cells(3, 0)[1]).all()
    assert all(len(ec.cells(m, 7)[0]) > 7 for m in ec.TARGET_COUNTS)


@pytest.mark.parametrize("jset", ec.JOINT_SETS + ec.FORM_SETS, ids=[s.id for s in ec.JOINT_SETS + ec.FORM_SETS])
def test_gpu_cases_do_not_depend_on_who_factored(jset):
    """For every joint set of tests/test_ehvi_gpu.py: the oracle in float64 with LAPACK's factors, with the kernels' row-by-row
    factors, and in ``np.longdouble`` agree to a tenth of the tolerance the device is held to, on every scored row - so a device
    miss is the device's.  Every scored row is finite.  The rows that do not factor are the labelled ones, target by target."""
    d = jset.build()
    lo, up = jset.cells()
    Sig, means = ec.sigmas(d)
    L_ref = np.stack([oo.lapack_factors(s) for s in Sig])
    L_row = np.stack([oo.rowwise_factors(s) for s in Sig])
    for t in range(jset.m):
        notpd = d.target_is_label(t, "notpd")
        assert np.array_equal(np.isnan(L_ref[t, :, 0, 0]), notpd) and np.array_equal(np.isnan(L_row[t, :, 0, 0]), notpd)
    live = d.scored
    assert live.sum() >= min(jset.N, 40) or jset.N == 1, (jset.id, int(live.sum()))
    assert jset.N == 1 or (d.notpd.sum() > d.target_is_label(0, "notpd").sum())  # rows that are not-PSD in SOME target only
    for log in (True, False):
        a = oe.scores_from_factors(log, means, L_ref, d.z, lo, up)[live]
        b = oe.scores_from_factors(log, means, L_row, d.z, lo, up)[live]
        c = oe.scores_from_factors(log, means[:, live], L_ref[:, live], d.z, lo, up, dtype=np.longdouble).astype(np.float64)
        assert np.isfinite(a).all(), (jset.id, log)
        if log:
            dev = max(float(np.abs(a - b).max()), float(np.abs(a - c).max()))
            assert dev < SCORE_ATOL / 10, (jset.id, dev)
        else:
            dev = max(oc.mc_ratio(b, a), oc.mc_ratio(c, a))
            assert dev < 0.1, (jset.id, dev)


@pytest.mark.parametrize("m,p", [(2, 3), (3, 7)])
def test_agreement_inputs_are_exchangeable_and_far_below_is_far_enough(m, p):
    """The guards of the device's agreement tests, on the oracle: permuting the pending points of ``exchangeable_inputs`` (with their
    base-sample columns) and replacing the last one by a point far below the reference point move no score by a tenth of the
    device's tolerance."""
    inp = ec.exchangeable_inputs(m, p)
    lo, up = ec.cells(m, 7)
    perm = np.random.default_rng(p).permutation(p)
    assert not np.array_equal(perm, np.arange(p))

    def score(log, x):
        mean, var, cross, mp, cpp, z = x
        return oe.joint_scores(log, mean, var, cross, mp, cpp, z, lo, up)

    for log in (True, False):
        a, b = score(log, inp), score(log, ec.permuted(inp, perm))
        c, e = score(log, ec.with_last_far_below(inp)), score(log, ec.without_last(inp))
        assert np.isfinite(a).all() and np.isfinite(c).all()
        if log:
            assert np.abs(a - b).max() < SCORE_ATOL / 10 and np.abs(c - e).max() < SCORE_ATOL / 10
        else:
            assert oc.mc_ratio(b, a) < 0.1 and oc.mc_ratio(c, e) < 0.1


# ---- host set-up -----------------------------------------------------------------------------------------------------------------------
def test_make_partitioning_validates_like_the_reference_and_decomposes_exactly():
    from baybe_amd.ehvi import make_partitioning

    ref = np.full(3, ec.REF)
    with pytest.raises(ValueError, match=r"Predictions must be a 2-D tensor, got shape \(3,\)"):
        make_partitioning(np.zeros(3), ref, None)
    with pytest.raises(ValueError, match=r"Reference point must be a 1-D tensor, got shape \(1, 3\)"):
        make_partitioning(np.zeros((4, 3)), ref[None, :], None)
    with pytest.raises(ValueError, match="Predictions dimensionality 2 does not match reference point dimensionality 3"):
        make_partitioning(np.zeros((4, 2)), ref, None)
    with pytest.raises(IncompatibilityError, match="alpha=0") as info:
        make_partitioning(np.zeros((4, 3)), ref, 1e-3)
    assert "BotorchRecommender" in str(info.value)
    with pytest.raises(IncompatibilityError, match="2 to 4 targets"):
        make_partitioning(np.zeros((4, 5)), np.zeros(5), None)
    for m in ec.TARGET_COUNTS:
        for k in ec.FRONT_SIZES:
            # the front and points it dominates (or that lie below the reference point) give the same cells
            P = ec.front(m, k)
            Y = np.vstack([P, P - 0.3, np.full((1, m), ec.REF - 1.0)]) if k else np.zeros((0, m))
            want = np.hstack(no.nondominated_cells(P, np.full(m, ec.REF)))
            for alpha in (None, 0, 0.0):
                lo, up = make_partitioning(Y, np.full(m, ec.REF), alpha)
                got = np.hstack([lo, up])
                assert got.shape == want.shape
                assert np.array_equal(got[np.lexsort(got.T)], want[np.lexsort(want.T)])


# ---- conversion -------------------------------------------------------------------------------------------------------------------------
def test_convert_acqf_refuses_by_default_and_converts_on_request():
    for name in ("qEHVI", "qLogEHVI", "qExpectedHypervolumeImprovement", "qLogExpectedHypervolumeImprovement"):
        with pytest.raises(IncompatibleAcquisitionFunctionError, match="ehvi='device'"):
            A.convert_acqf(name)
        with pytest.raises(IncompatibleAcquisitionFunctionError, match="not available on this path"):
            A.convert_acqf(name, ehvi="refuse")
    with pytest.raises(IncompatibleAcquisitionFunctionError):
        A.convert_acqf(A.qLogEHVI())  # our own instance as well
    with pytest.raises(IncompatibleAcquisitionFunctionError):
        A.convert_acqf("qKG", ehvi="device")  # the setting opens nothing else
    assert A.qEHVI is A.qExpectedHypervolumeImprovement and A.qLogEHVI is A.qLogExpectedHypervolumeImprovement
    for name, cls in (("qEHVI", A.qEHVI), ("qLogEHVI", A.qLogEHVI), ("qExpectedHypervolumeImprovement", A.qEHVI),
                      ("qLogExpectedHypervolumeImprovement", A.qLogEHVI)):
        got = A.convert_acqf(name, ehvi="device")
        assert type(got) is cls and got.kind == cls.abbreviation and got.alpha is None and got.reference_point is None
        assert got.n_mc_samples == 128 and not hasattr(got, "prune_baseline")
        assert got.supports_multi_output and got.supports_batching and got.supports_pending_experiments
    own = A.qLogEHVI(reference_point=(0.0, 1), alpha=0, n_mc_samples=64)
    assert A.convert_acqf(own, ehvi="device") is own and own.reference_point == (0.0, 1.0) and own.alpha == 0.0
    standin = type("qExpectedHypervolumeImprovement", (), {"reference_point": 0.2, "alpha": 0.0})()
    got = A.convert_acqf(standin, ehvi="device")
    assert type(got) is A.qEHVI and got.reference_point == 0.2 and got.alpha == 0.0
    # what was converted before still is, under either setting
    for ehvi in ("refuse", "device"):
        assert type(A.convert_acqf("qLogNEHVI", ehvi=ehvi)) is A.qLogNEHVI and type(A.convert_acqf("qEI", ehvi=ehvi)) is A.qEI


def test_convert_acqf_takes_the_references_own_objects():
    from _reference import reference_baybe

    reference_baybe()
    from baybe.acquisition.acqfs import qExpectedHypervolumeImprovement, qLogExpectedHypervolumeImprovement

    got = A.convert_acqf(qLogExpectedHypervolumeImprovement(reference_point=[0.5, 2.0], alpha=0.0), ehvi="device")
    assert type(got) is A.qLogEHVI and got.reference_point == (0.5, 2.0) and got.alpha == 0.0
    got = A.convert_acqf(qExpectedHypervolumeImprovement(), ehvi="device")
    assert type(got) is A.qEHVI and got.reference_point is None and got.alpha is None
    with pytest.raises(IncompatibleAcquisitionFunctionError, match="ehvi='device'"):
        A.convert_acqf(qExpectedHypervolumeImprovement())


def test_recommender_field():
    from baybe_amd.recommenders import HipBotorchRecommender as R

    assert R().ehvi == "refuse" and R(ehvi="device").ehvi == "device"
    with pytest.raises(ValueError, match="ehvi"):
        R(ehvi="host")
    with pytest.raises(IncompatibleAcquisitionFunctionError, match="ehvi='device'"):
        R(acquisition_function="qLogEHVI")
    rec = R(ehvi="device", acquisition_function="qLogEHVI")
    assert type(rec.acquisition_function) is A.qLogEHVI
    assert type(R(acquisition_function="qEHVI", ehvi="device").acquisition_function) is A.qEHVI  # whatever the keyword order


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_fitted(monkeypatch):
    import pandas as pd

    from _baybe_shim import NumericalTarget, ParetoObjective
    from baybe_amd import engine as engine_mod
    from baybe_amd.exceptions import IncompatibleSurrogateError
    from baybe_amd.forest import HipRandomForestSurrogate
    from baybe_amd.linear import HipBayesianLinearSurrogate
    from baybe_amd.recommenders import HipBotorchRecommender as R

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the refusal")

    monkeypatch.setattr(engine_mod, "HipGP", NoEngine)
    space, meas, objective, names, signs = ec.campaign_problem(2)
    exp = space.discrete.exp_rep
    for kind in ("qEHVI", "qLogEHVI"):
        with pytest.raises(IncompatibilityError, match="alpha=0") as info:
            R(ehvi="device", acquisition_function=getattr(A, kind)(alpha=0.01)).recommend(1, space, objective, meas)
        assert "BotorchRecommender" in str(info.value)
        # 1 + pending + batch_size > 8
        with pytest.raises(IncompatibilityError, match="qLogNEHVI") as info:
            R(ehvi="device", acquisition_function=kind).recommend(8, space, objective, meas)
        assert "limit of 8" in str(info.value)
        with pytest.raises(IncompatibilityError, match="qLogNEHVI"):
            R(ehvi="device", acquisition_function=kind).recommend(4, space, objective, meas, pending_experiments=exp.iloc[:4])
        with pytest.raises(IncompatibilityError, match="Row shards"):
            R(ehvi="device", acquisition_function=kind, shard=SimpleNamespace(world=2, rank=0, N_total=200, start=0, stop=100)
              ).recommend(1, space, objective, meas)
        hybrid = type(space)(space.discrete)
        hybrid.continuous = SimpleNamespace(is_empty=False, comp_rep_bounds=pd.DataFrame({"c": [0.0, 1.0]}))
        with pytest.raises(IncompatibilityError, match="hybrid / continuous"):
            R(ehvi="device", acquisition_function=kind).recommend(1, hybrid, objective, meas)
        for surrogate in (HipRandomForestSurrogate(), HipBayesianLinearSurrogate()):
            with pytest.raises(IncompatibleSurrogateError, match="single-output surrogate"):
                R(ehvi="device", acquisition_function=kind, surrogate_model=surrogate).recommend(1, space, objective, meas)
        # a transformed target under a ParetoObjective: what the noisy pair refuses
        bent = NumericalTarget("t0")
        bent.transformation = oc._tr("BellTransformation", center=0.0, sigma=1.0)
        with pytest.raises(IncompatibilityError):
            R(ehvi="device", acquisition_function=kind).recommend(1, space, ParetoObjective([bent, NumericalTarget("t1")]), meas)
        # a single target
        from _baybe_shim import SingleTargetObjective

        with pytest.raises(IncompatibleAcquisitionFunctionError, match="multi-output"):
            R(ehvi="device", acquisition_function=kind).recommend(1, space, SingleTargetObjective(NumericalTarget("t0")), meas)
    five = ParetoObjective([NumericalTarget(f"u{j}") for j in range(5)])
    meas5 = meas.assign(**{f"u{j}": np.linspace(0, 1, len(meas)) for j in range(5)})
    with pytest.raises(IncompatibilityError, match="2 to 4 targets"):
        R(ehvi="device", acquisition_function="qLogEHVI").recommend(1, space, five, meas5)


# ---- the end-to-end campaign's picks are decided by more than the tolerance ----------------------------------------------------------------
_FITTED: dict = {}


def _campaign_models(m):
    """The oracle's own fit of the campaign's targets, once per m (shared, unchanged)."""
    from oracle import gp_oracle as go

    if m not in _FITTED:
        space, meas, objective, names, signs = ec.campaign_problem(m)
        X_all = meas[["x0", "x1", "x2"]].to_numpy(float)
        spec = go.GPSpec.baybe_default(3, np.zeros(3), np.ones(3))
        _FITTED[m] = [go.fit_gp(spec, X_all, meas[n].to_numpy()) for n in names]
    return _FITTED[m]


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("log", [True, False], ids=["qLogEHVI", "qEHVI"])
@pytest.mark.parametrize("pending", [False, True], ids=["", "pending"])
def test_campaign_picks_are_separated_by_a_hundred_tolerances(m, log, pending):
    """tests/test_ehvi_gpu.py compares picks: at every greedy step the oracle's best and second-best scores differ by more than
    100 tolerances (the oracle's own fit here, the device's hyper-parameters there, where the same assertion is repeated)."""
    space, meas, objective, names, signs = ec.campaign_problem(m)
    X_all = meas[["x0", "x1", "x2"]].to_numpy(float)
    models = _campaign_models(m)
    Xc = space.discrete.exp_rep.to_numpy(float)
    ref = ec.campaign_ref_point(meas, names, signs)
    pend = Xc[[ec.CAMPAIGN_PENDING_ROW]] if pending else None
    idx, vals, gaps = oe.greedy(log, models, signs, Xc, ec.CAMPAIGN_BATCH, ec.next_sampler_seed(ec.CAMPAIGN_SEED), X_all, ref, pending=pend)
    assert len(set(idx)) == ec.CAMPAIGN_BATCH
    for v, g in zip(vals, gaps):
        assert g > 100 * ec.gap_tolerance(log, v), (idx, vals, gaps)
