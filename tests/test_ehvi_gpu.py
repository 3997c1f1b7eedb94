"""The qEHVI / qLogEHVI kernels of baybe_amd/csrc/bbh_ehvi.hip on the device, against tests/_oracle_ehvi.py.

  q' = 1     ``bbh_ehvi_q1``: N = 1 and 257, S = 1, 33 and 128 (one, three and eight sample slices), m = 2, 3 and 4, the cell lists of
             fronts of 0, 1 and 7 points, both forms, rows that need the 1 x 1 jitter, one masked row
  joint      ``bbh_ehvi_pending``: per-target synthetic joint statistics (tests/_ehvi_cases.py), 130 rows at (m, p) = (2, 1), (3, 2),
             (4, 3), (2, 7) in the LDS form (asked for by name: left to itself the library takes the workspace form, which measured
             faster) and (4, 7) in the workspace form, and one single row; NaN exactly on the rows that do not factor, -inf exactly
             on the masked rows
  forms      the workspace form forced equals the LDS form bit for bit; the LDS form where it does not fit, p = 8 and m = 5 are
             bad-arguments errors and launch nothing
  agreement  permuted pending points; a pending point far below the reference point; two runs give equal bits
  end to end ``HipBotorchRecommender(ehvi="device")``: the picks are the oracle's greedy picks

Bounds: qLogEHVI ``_joint_cases.SCORE_ATOL``; qEHVI MC_RTOL / MC_ATOL of tests/test_joint_batch_gpu.py
(``_objective_cases.mc_ratio`` <= 1).  The inputs are guarded by tests/test_ehvi_cpu.py.

Observed on an MI355X (profiles/ehvi_observed_deviations.json, KERNELS.md section 4.14), qLogEHVI absolute / qEHVI in units of its
tolerance: q' = 1 6.3e-12 / 2.5e-7, joint 9.6e-13 / 9.6e-5, permuted 8.9e-16 / 2.2e-8, far below 0 / 1.6e-8, recommender
5.6e-13 / 6.6e-7."""

import numpy as np
import pytest

import _ehvi_cases as ec
import _objective_cases as oc
import _oracle_ehvi as oe
import _oracle_objective as oo
from _joint_cases import SCORE_ATOL

pytestmark = pytest.mark.gpu
FORMS = ((True, "qLogEHVI"), (False, "qEHVI"))


@pytest.fixture(scope="module")
def gp():
    from baybe_amd import engine

    g = engine.HipGP(0)
    yield g
    g.close()


def _dev(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _record(name, value, tol):
    from conftest import record_deviation

    print(f"{name}: observed {value:.3e} (tolerance {tol:.1e})")
    record_deviation(f"ehvi/{name}", value, tol)


def _deviation(log, got, ref):
    """(deviation in units of the form's tolerance, tolerance as recorded)."""
    if log:
        return (float(np.abs(got - ref).max()) if len(ref) else 0.0), SCORE_ATOL
    return oc.mc_ratio(got, ref), 1.0


def _joint(gp, log, inputs, cells, alive=None, form=-1):
    mean, var, cross, mp, cpp, z = inputs
    return gp.ehvi_acq(log, _dev(mean), _dev(var), cells, z, None if alive is None else _dev(alive), cross=_dev(cross), stats=(mp, cpp),
                       form=form).cpu().numpy()


@pytest.mark.parametrize("N,S", ec.Q1_SHAPES, ids=[f"N{n}-S{s}" for n, s in ec.Q1_SHAPES])
def test_q1_every_form_cell_list_and_target_count(gp, N, S):
    failures = []
    worst = {name: 0.0 for _, name in FORMS}
    for m in ec.TARGET_COUNTS:
        mean, var, z, alive = ec.q1_inputs(N, S, m)
        live = alive.astype(bool)
        dm, dv, da = _dev(mean), _dev(var), _dev(alive)
        for k in ec.FRONT_SIZES:
            lo, up = ec.cells(m, k)
            for log, name in FORMS:
                got = gp.ehvi_acq(log, dm, dv, (lo, up), z, da).cpu().numpy()
                ref = oe.q1_scores(log, mean, var, z, lo, up)
                assert np.isfinite(ref[live]).all(), (m, k, name)
                if not (np.isneginf(got[~live]).all() and np.isfinite(got[live]).all()):
                    failures.append((m, k, name, "masked / non-finite rows"))
                    continue
                dev, tol = _deviation(log, got[live], ref[live])
                worst[name] = max(worst[name], dev)
                if not dev <= tol:
                    failures.append((m, k, name, dev))
    for log, name in FORMS:
        _record(f"q1[N={N},S={S},{name}]", worst[name], SCORE_ATOL if log else 1.0)
    assert not failures, failures


@pytest.mark.parametrize("jset", ec.JOINT_SETS, ids=[s.id for s in ec.JOINT_SETS])
def test_joint_both_forms(gp, jset):
    d = jset.build()
    lo, up = jset.cells()
    Sig, means = ec.sigmas(d)
    L = np.stack([oo.lapack_factors(s) for s in Sig])
    inputs = (d.mean, d.var, d.cross, d.mean_p, d.cov_pp, d.z)
    failures = []
    for log, name in FORMS:
        got = _joint(gp, log, inputs, (lo, up), d.alive, form=jset.form if jset.form == 0 else -1)  # (-1: the library takes the workspace)
        assert gp.ehvi_last_form() == jset.form, (jset.id, gp.ehvi_last_form())
        ref = oe.scores_from_factors(log, means, L, d.z, lo, up)
        ec.compare_rows(got, d, f"{jset.id}/{name}")  # NaN = notpd rows (in any target), -inf = masked rows
        dev, tol = _deviation(log, got[d.scored], ref[d.scored])
        _record(f"joint[{jset.id},{name}]", dev, tol)
        if not dev <= tol:
            failures.append((name, dev))
    assert not failures, failures


@pytest.mark.parametrize("jset", ec.FORM_SETS, ids=[s.id for s in ec.FORM_SETS])
def test_workspace_form_equals_lds_form_bit_for_bit(gp, jset):
    d = jset.build()
    inputs = (d.mean, d.var, d.cross, d.mean_p, d.cov_pp, d.z)
    for log, name in FORMS:
        out = []
        for form in (0, 1):
            out.append(_joint(gp, log, inputs, jset.cells(), d.alive, form=form))
            assert gp.ehvi_last_form() == form
        ec.compare_rows(out[0], d, f"{jset.id}/{name}")
        assert np.array_equal(out[0], out[1], equal_nan=True), (jset.id, name)


def test_bad_arguments_launch_nothing(gp):
    from baybe_amd._lib import EHVI_MAX_Q, HipError

    small, big = ec.FORM_SETS[0], ec.JOINT_SETS[4]
    assert (big.m, big.p, big.form) == (4, 7, 1) and EHVI_MAX_Q == 8
    ds = small.build()
    _joint(gp, False, (ds.mean, ds.var, ds.cross, ds.mean_p, ds.cov_pp, ds.z), small.cells(), form=0)
    assert gp.ehvi_last_form() == 0
    d = big.build()
    with pytest.raises(HipError, match="bad arguments"):  # the LDS form where it does not fit
        _joint(gp, False, (d.mean, d.var, d.cross, d.mean_p, d.cov_pp, d.z), big.cells(), form=0)
    assert gp.ehvi_last_form() == 0  # nothing was launched: still the form of the call before
    rng = np.random.default_rng(0)
    N, S = 5, 4
    for m, p in ((2, 8), (5, 1)):  # nine points; five targets
        lo = np.full((1, m), ec.REF)
        args = (rng.standard_normal((m, N)), np.ones((m, N)), np.zeros((m, N, p)), np.zeros((m, p)), np.stack([np.eye(p)] * m),
                rng.standard_normal((S, p + 1, m)))
        with pytest.raises(HipError, match="bad arguments"):
            _joint(gp, True, args, (lo, np.full((1, m), np.inf)))
        assert gp.ehvi_last_form() == 0
    with pytest.raises(HipError, match="bad arguments"):
        gp.ehvi_acq(True, _dev(np.zeros((5, N))), _dev(np.ones((5, N))), (np.full((1, 5), ec.REF), np.full((1, 5), np.inf)),
                    rng.standard_normal((S, 5)))
    with pytest.raises(HipError, match="bad arguments"):  # an empty cell (upper bound not above the lower one)
        gp.ehvi_acq(True, _dev(np.zeros((2, N))), _dev(np.ones((2, N))), (np.zeros((1, 2)), np.zeros((1, 2))), rng.standard_normal((S, 2)))


# ---- agreement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,p", [(2, 3), (3, 7)])
def test_permuted_and_far_below_pending_points(gp, m, p):
    inp = ec.exchangeable_inputs(m, p)
    cells = ec.cells(m, 7)
    perm = np.random.default_rng(p).permutation(p)
    failures = []
    for log, name in FORMS:
        a, b = _joint(gp, log, inp, cells), _joint(gp, log, ec.permuted(inp, perm), cells)
        c, e = _joint(gp, log, ec.with_last_far_below(inp), cells), _joint(gp, log, ec.without_last(inp), cells)
        assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all() and np.isfinite(e).all()
        dev_perm, tol = _deviation(log, b, a)
        dev_far, _ = _deviation(log, c, e)
        _record(f"permuted[m={m},p={p},{name}]", dev_perm, tol)
        _record(f"far-below[m={m},p={p},{name}]", dev_far, tol)
        if not (dev_perm <= tol and dev_far <= tol):
            failures.append((name, dev_perm, dev_far))
    # ... and q' = 2 against the q' = 1 kernel
    one = ec.exchangeable_inputs(m, 1)
    for log, name in FORMS:
        c = _joint(gp, log, ec.with_last_far_below(one), cells)
        e = gp.ehvi_acq(log, _dev(one[0]), _dev(one[1]), cells, np.ascontiguousarray(one[5][:, 0, :])).cpu().numpy()
        dev, tol = _deviation(log, c, e)
        _record(f"far-below[m={m},p=1,{name}]", dev, tol)
        if not dev <= tol:
            failures.append((name, "q1", dev))
    assert not failures, failures


def test_two_runs_give_equal_bits(gp):
    jset = ec.JOINT_SETS[1]
    d = jset.build()
    inputs = (d.mean, d.var, d.cross, d.mean_p, d.cov_pp, d.z)
    mean, var, z, alive = ec.q1_inputs(257, 128, 3)
    for log, name in FORMS:
        a, b = _joint(gp, log, inputs, jset.cells(), d.alive), _joint(gp, log, inputs, jset.cells(), d.alive)
        assert np.array_equal(a, b, equal_nan=True), name
        a = gp.ehvi_acq(log, _dev(mean), _dev(var), ec.cells(3, 7), z, _dev(alive)).cpu().numpy()
        b = gp.ehvi_acq(log, _dev(mean), _dev(var), ec.cells(3, 7), z, _dev(alive)).cpu().numpy()
        assert np.array_equal(a, b), name
        # equal rows tie bit for bit, whatever else is scored with them
        two = gp.ehvi_acq(log, _dev(mean[:, [7, 7]]), _dev(var[:, [7, 7]]), ec.cells(3, 7), z).cpu().numpy()
        assert two[0] == two[1] == a[7], name


# ---- through the recommender ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pending", [False, True], ids=["", "pending"])
@pytest.mark.parametrize("m", [2, 3])
def test_recommender_end_to_end(m, pending):
    """200 candidates, m targets (the second minimised), batch 3, with and without one pending experiment: under the device's fitted
    hyper-parameters the picks are the oracle's greedy picks, for qLogEHVI and qEHVI; the read-backs match; the default refuses."""
    from baybe_amd.exceptions import IncompatibleAcquisitionFunctionError
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go

    space, meas, objective, names, signs = ec.campaign_problem(m)
    exp = space.discrete.exp_rep
    Xc, X_all = exp.to_numpy(float), meas[["x0", "x1", "x2"]].to_numpy(float)
    pend_df = exp.iloc[[ec.CAMPAIGN_PENDING_ROW]] if pending else None
    pend = Xc[[ec.CAMPAIGN_PENDING_ROW]] if pending else None
    ref = ec.campaign_ref_point(meas, names, signs)
    with pytest.raises(IncompatibleAcquisitionFunctionError, match="ehvi='device'"):
        HipBotorchRecommender(acquisition_function="qLogEHVI")
    models = None
    for log, name in FORMS:
        rec = HipBotorchRecommender(ehvi="device", acquisition_function=name)
        seed = ec.next_sampler_seed(ec.CAMPAIGN_SEED)
        got = rec.recommend(ec.CAMPAIGN_BATCH, space, objective, meas, pending_experiments=pend_df)
        if models is None:  # (the fit does not depend on the acquisition function)
            models = []
            for nm, sub in zip(names, rec._surrogate_model.models):
                prm = sub.engine.params
                models.append(go.GPModel(go.GPSpec.baybe_default(3, np.zeros(3), np.ones(3)), go.GPParams(prm.lengthscale, prm.noise, prm.mean),
                                         X_all, meas[nm].to_numpy()))
        idx, vals, gaps = oe.greedy(log, models, signs, Xc, ec.CAMPAIGN_BATCH, seed, X_all, ref, pending=pend)
        assert all(g > 100 * ec.gap_tolerance(log, v) for v, g in zip(vals, gaps)), (name, vals, gaps)
        assert got.index.tolist() == exp.index[idx].tolist(), name
        lo, up = oe.model_cells(models, signs, X_all, ref)
        glo, gup = rec._scorer.cells()
        assert glo.shape == lo.shape and np.allclose(np.sort(glo, axis=0), np.sort(lo, axis=0), atol=1e-9)
        seed = ec.next_sampler_seed(5)
        acq = rec.acquisition_values(exp.iloc[:60], space, objective, meas, pending_experiments=pend_df).to_numpy()
        want = oe.model_scores(log, models, signs, Xc[:60], pend, oe.base_samples(128, 1 + int(pending), m, seed), lo, up)
        dev_acq, tol = _deviation(log, acq, want)
        seed = ec.next_sampler_seed(6)
        jv = rec.joint_acquisition_value(exp.iloc[[3, 140, 77]], space, objective, meas, pending_experiments=pend_df)
        rows = Xc[[3, 140, 77]]
        rest = rows[1:] if pend is None else np.vstack([rows[1:], pend])
        want_j = oe.model_scores(log, models, signs, rows[:1], rest, oe.base_samples(128, 3 + int(pending), m, seed), lo, up)
        dev_j, _ = _deviation(log, np.array([jv]), want_j)
        _record(f"recommender[m={m},{'pending,' if pending else ''}{name},acquisition_values]", dev_acq, tol)
        _record(f"recommender[m={m},{'pending,' if pending else ''}{name},joint_acquisition_value]", dev_j, tol)
        assert dev_acq <= tol and dev_j <= tol, (name, dev_acq, dev_j)
