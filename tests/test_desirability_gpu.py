"""The desirability kernels of baybe_amd/csrc/bbh_desirability.hip on the device, against tests/_oracle_desirability.py.

  q = 1      ``bbh_desirability_q1``: N = 1 and 257, S = 1, 33 and 512, T = 2, 3 and 8, both scalarisers, every MC kind, rows that
             need the 1 x 1 jitter, one masked row
  joint      ``bbh_desirability_pending``: per-target synthetic joint statistics (tests/_desirability_cases.py), 130 rows at
             (T, p) = (2, 15), (3, 1), (8, 2) in the LDS form and (8, 15) in the workspace form, and one single row; NaN exactly on
             the rows that do not factor, -inf exactly on the masked rows
  forms      the workspace form forced equals the LDS form bit for bit; the LDS form where it does not fit is a bad-arguments error
  agreement  weights (1, 0) under the arithmetic mean reproduce ``mc_acq(objective=prog_0)``; permuted targets give the same scores
  end to end ``HipBotorchRecommender(desirability="device")``: the picks are the oracle's greedy picks

Bounds: qLogEI ``_joint_cases.SCORE_ATOL``; the other kinds MC_RTOL / MC_ATOL of tests/test_joint_batch_gpu.py
(``_objective_cases.mc_ratio`` <= 1).  The joint inputs are guarded by
tests/test_desirability_cpu.py::test_gpu_cases_do_not_depend_on_who_factored."""

import numpy as np
import pytest

import _desirability_cases as dc
import _objective_cases as oc
import _oracle_desirability as od
import _oracle_objective as oo
from _joint_cases import SCORE_ATOL

pytestmark = pytest.mark.gpu


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
    record_deviation(f"desirability/{name}", value, tol)


def _deviation(kind, got, ref):
    """(deviation in units of the kind's tolerance, tolerance as recorded)."""
    if kind == "qLogEI":
        return (float(np.abs(got - ref).max()) if len(ref) else 0.0), SCORE_ATOL
    return oc.mc_ratio(got, ref), 1.0


@pytest.mark.parametrize("N,S", dc.Q1_SHAPES, ids=[f"N{n}-S{s}" for n, s in dc.Q1_SHAPES])
def test_q1_every_kind_scalariser_and_target_count(gp, N, S):
    failures = []
    worst = {k: 0.0 for k in dc.MC_KINDS}
    for T in dc.TARGET_COUNTS:
        mean, var, z, alive = dc.q1_inputs(N, S, T)
        live = alive.astype(bool)
        dm, dv, da = _dev(mean), _dev(var), _dev(alive)
        for scal in dc.SCALARIZERS:
            des = dc.description(T, scal)
            prog = dc.product_program(des)
            bf = dc.case_best_f(des, mean)
            for kind in dc.MC_KINDS:
                got = gp.desirability_acq(prog, kind, dm, dv, z, bf, dc.BETA, da).cpu().numpy()
                ref = od.q1_scores(kind, des, mean, var, z, bf, dc.BETA)
                assert np.isfinite(ref[live]).all(), (T, scal, kind)
                if not (np.isneginf(got[~live]).all() and np.isfinite(got[live]).all()):
                    failures.append((T, scal, kind, "masked / non-finite rows"))
                    continue
                dev, tol = _deviation(kind, got[live], ref[live])
                worst[kind] = max(worst[kind], dev)
                if not dev <= tol:
                    failures.append((T, scal, kind, dev))
    for kind in dc.MC_KINDS:
        _record(f"q1[N={N},S={S},{kind}]", worst[kind], SCORE_ATOL if kind == "qLogEI" else 1.0)
    assert not failures, failures


@pytest.mark.parametrize("jset", dc.JOINT_SETS, ids=[s.id for s in dc.JOINT_SETS])
def test_joint_every_kind_and_scalariser(gp, jset):
    d = jset.build()
    Sig, means = d.sigmas()
    L = np.stack([oo.lapack_factors(s) for s in Sig])
    dm, dv, dx, da = _dev(d.mean), _dev(d.var), _dev(d.cross), _dev(d.alive)
    failures = []
    worst = {k: 0.0 for k in dc.MC_KINDS}
    for scal in dc.SCALARIZERS:
        des = dc.description(jset.T, scal)
        prog = dc.product_program(des)
        bf = dc.case_best_f(des, d.mean)
        for kind in dc.MC_KINDS:
            got = gp.desirability_acq(prog, kind, dm, dv, d.z, bf, dc.BETA, da, cross=dx, stats=(d.mean_p, d.cov_pp)).cpu().numpy()
            assert gp.desirability_last_form() == jset.form, (jset.id, gp.desirability_last_form())
            ref = od.scores_from_factors(kind, des, means, L, d.z, bf, dc.BETA)
            dc.compare_rows(got, d, f"{jset.id}/{scal}/{kind}")  # NaN = notpd rows (in any target), -inf = masked rows
            dev, tol = _deviation(kind, got[d.scored], ref[d.scored])
            worst[kind] = max(worst[kind], dev)
            if not dev <= tol:
                failures.append((scal, kind, dev))
    for kind in dc.MC_KINDS:
        _record(f"joint[{jset.id},{kind}]", worst[kind], SCORE_ATOL if kind == "qLogEI" else 1.0)
    assert not failures, failures


@pytest.mark.parametrize("jset", dc.FORM_SETS, ids=[s.id for s in dc.FORM_SETS])
def test_workspace_form_equals_lds_form_bit_for_bit(gp, jset):
    d = jset.build()
    dm, dv, dx, da = _dev(d.mean), _dev(d.var), _dev(d.cross), _dev(d.alive)
    for scal in dc.SCALARIZERS:
        des = dc.description(jset.T, scal)
        prog = dc.product_program(des)
        bf = dc.case_best_f(des, d.mean)
        for kind in dc.MC_KINDS:
            out = []
            for form in (0, 1):
                out.append(gp.desirability_acq(prog, kind, dm, dv, d.z, bf, dc.BETA, da, cross=dx, stats=(d.mean_p, d.cov_pp),
                                               form=form).cpu().numpy())
                assert gp.desirability_last_form() == form
            dc.compare_rows(out[0], d, f"{jset.id}/{scal}/{kind}")
            assert np.array_equal(out[0], out[1], equal_nan=True), (jset.id, scal, kind)


def test_lds_form_that_does_not_fit_is_a_bad_arguments_error(gp):
    from baybe_amd._lib import HipError

    small, big = dc.FORM_SETS[0], dc.JOINT_SETS[3]
    assert (big.T, big.p) == (8, 15)
    ds = small.build()
    des = dc.description(small.T, "MEAN")
    gp.desirability_acq(dc.product_program(des), "qEI", _dev(ds.mean), _dev(ds.var), ds.z, 0.0, dc.BETA, None, cross=_dev(ds.cross),
                        stats=(ds.mean_p, ds.cov_pp), form=0)
    assert gp.desirability_last_form() == 0
    d = big.build()
    des = dc.description(big.T, "MEAN")
    with pytest.raises(HipError, match="bad arguments"):
        gp.desirability_acq(dc.product_program(des), "qEI", _dev(d.mean), _dev(d.var), d.z, 0.0, dc.BETA, None, cross=_dev(d.cross),
                            stats=(d.mean_p, d.cov_pp), form=0)
    assert gp.desirability_last_form() == 0  # nothing was launched: still the form of the call before


# ---- agreement with the single-target path -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agree_inputs():
    """Ordinary rows only (every target factors as it stands): (mean, var [2, N]; per p: cross, mean_p, cov_pp, z)."""
    from _joint_cases import JointCase

    out = {}
    for p in dc.AGREE_P:
        if p == 0:
            mean, var, z, _ = dc.q1_inputs(257, 33, 2)
            out[p] = (mean, np.abs(var) + 0.01, None, None, None, z)
            continue
        ds = [JointCase(p, 64, 130, 1.0, s).build() for s in (0, 4)]
        rows = ds[0].is_label("ordinary")
        z = od.base_samples(64, p + 1, 2, 11)
        out[p] = (np.stack([d.mean[rows] for d in ds]), np.stack([d.var[rows] for d in ds]), np.stack([d.cross[rows] for d in ds]),
                  np.stack([d.mean_p for d in ds]), np.stack([d.cov_pp for d in ds]), z)
    return out


@pytest.mark.parametrize("p", dc.AGREE_P, ids=lambda p: f"q{p + 1}")
def test_weights_one_zero_reproduce_the_single_target_kernels(gp, agree_inputs, p):
    """The arithmetic mean with weights (1, 0) is the first target's program alone: the scores of
    ``mc_acq(objective=prog_0)`` on the first target's statistics and base-sample column, within the MC tolerance."""
    from baybe_amd.desirability import DesirabilityProgram
    from baybe_amd.objective import ObjectiveProgram

    mean, var, cross, mp, cpp, z = agree_inputs[p]
    dm, dv = _dev(mean), _dev(var)
    dx = None if p == 0 else _dev(cross)
    failures = []
    worst = {k: 0.0 for k in dc.MC_KINDS}
    for first in ("bell", "triangular-min"):
        progs = (ObjectiveProgram(tuple(oc.PROGRAMS[first])), ObjectiveProgram(tuple(oc.PROGRAMS["sigmoid"])))
        des = DesirabilityProgram(progs, (1.0, 0.0), "MEAN")
        bf = oc.case_best_f(oc.PROGRAMS[first], mean[0])
        for kind in dc.MC_KINDS:
            if p == 0:
                new = gp.desirability_acq(des, kind, dm, dv, z, bf, dc.BETA)
                old = gp.mc_acq(kind, dm[0].contiguous(), dv[0].contiguous(), np.ascontiguousarray(z[:, 0]), bf, beta=dc.BETA, objective=progs[0])
            else:
                new = gp.desirability_acq(des, kind, dm, dv, z, bf, dc.BETA, cross=dx, stats=(mp, cpp))
                old = gp.mc_acq(kind, dm[0].contiguous(), dv[0].contiguous(), np.ascontiguousarray(z[:, :, 0]), bf, beta=dc.BETA,
                                cross=dx[0].contiguous(), objective=progs[0], stats=(mp[0], cpp[0]))
            new, old = new.cpu().numpy(), old.cpu().numpy()
            assert np.isfinite(old).all() and np.isfinite(new).all(), (first, kind)
            dev, tol = _deviation(kind, new, old)
            worst[kind] = max(worst[kind], dev)
            if not dev <= tol:
                failures.append((first, kind, dev))
    for kind in dc.MC_KINDS:
        _record(f"single-target[q'={p + 1},{kind}]", worst[kind], SCORE_ATOL if kind == "qLogEI" else 1.0)
    assert not failures, failures


@pytest.mark.parametrize("jset", [dc.JOINT_SETS[1], dc.JOINT_SETS[2]], ids=lambda s: s.id)
def test_permuted_targets_give_the_same_scores(gp, jset):
    from baybe_amd.desirability import DesirabilityProgram

    d = jset.build()
    perm = np.random.default_rng(jset.T).permutation(jset.T)
    assert not np.array_equal(perm, np.arange(jset.T))
    failures = []
    for scal in dc.SCALARIZERS:
        des = dc.description(jset.T, scal)
        prog = dc.product_program(des)
        permuted = DesirabilityProgram(tuple(prog.programs[t] for t in perm), tuple(prog.normalized_weights[t] for t in perm), scal)
        bf = dc.case_best_f(des, d.mean)
        for kind in dc.MC_KINDS:
            a = gp.desirability_acq(prog, kind, _dev(d.mean), _dev(d.var), d.z, bf, dc.BETA, _dev(d.alive), cross=_dev(d.cross),
                                    stats=(d.mean_p, d.cov_pp)).cpu().numpy()
            b = gp.desirability_acq(permuted, kind, _dev(d.mean[perm]), _dev(d.var[perm]), np.ascontiguousarray(d.z[:, :, perm]), bf, dc.BETA,
                                    _dev(d.alive), cross=_dev(d.cross[perm]), stats=(d.mean_p[perm], d.cov_pp[perm])).cpu().numpy()
            dc.compare_rows(b, d, f"{jset.id}/{scal}/{kind}/permuted")
            dev, tol = _deviation(kind, b[d.scored], a[d.scored])
            _record(f"permuted[{jset.id},{scal},{kind}]", dev, tol)
            if not dev <= tol:
                failures.append((scal, kind, dev))
    assert not failures, failures


# ---- through the recommender ---------------------------------------------------------------------------------------------------------
def _next_sampler_seed(seed_value):
    import torch

    torch.manual_seed(seed_value)
    s = int(torch.randint(0, 1000000, (1,)).item())
    torch.manual_seed(seed_value)
    return s


@pytest.mark.parametrize("scalarizer", ["GEOM_MEAN", "MEAN"])
def test_recommender_end_to_end(scalarizer):
    """216 candidates, 2 targets (a ramp, a minimised ramp), one row measured for the first target only, batch 3: the picks are the
    oracle's greedy picks under the device's fitted hyper-parameters; the read-backs match; the default setting still refuses."""
    from _baybe_shim import NumericalDiscreteParameter, SearchSpace
    from baybe_amd.desirability import desirability_program
    from baybe_amd.exceptions import IncompatibilityError
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go

    rng = np.random.default_rng(8)
    vals = np.arange(6) / 5.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])
    exp = space.discrete.exp_rep
    assert len(exp) == 216
    meas = exp.iloc[rng.choice(len(exp), 20, replace=False)].copy()
    Xm = meas[["x0", "x1", "x2"]].to_numpy(float)
    meas["gain"] = 100.0 * np.exp(-((Xm - 0.4) ** 2).sum(1)) + 0.5 * rng.standard_normal(len(Xm))
    meas["cost"] = 3.0 + 5.0 * Xm.sum(1) + 0.1 * rng.standard_normal(len(Xm))
    meas.loc[meas.index[4], "cost"] = np.nan
    cost = dc.ramp_target("cost", 3.0, 18.0)
    cost.minimize = True
    obj = dc.DesirabilityObjective([dc.ramp_target("gain", 20.0, 100.0), cost], weights=(2.0, 1.0), scalarizer=scalarizer)
    des = od.from_product(desirability_program(obj))
    assert des.programs[1][-1] == ("AFFINE", (-1.0, 1.0))
    with pytest.raises(IncompatibilityError, match="scalarise"):
        HipBotorchRecommender().recommend(3, space, obj, meas)
    rec = HipBotorchRecommender(desirability="device")
    seed = _next_sampler_seed(1337)
    got = rec.recommend(3, space, obj, meas)
    models = []
    for name, sub in zip(("gain", "cost"), rec._surrogate_model.models):
        rows = meas[~meas[name].isna()]
        prm = sub.engine.params
        models.append(go.GPModel(go.GPSpec.baybe_default(3, np.zeros(3), np.ones(3)), go.GPParams(prm.lengthscale, prm.noise, prm.mean),
                                 rows[["x0", "x1", "x2"]].to_numpy(float), rows[name].to_numpy()))
    assert [len(m.X_train) for m in models] == [20, 19]
    Xc = exp.to_numpy(float)
    idx, _ = od.greedy(models, Xc, 3, seed, des, Xm)
    assert got.index.tolist() == exp.index[idx].tolist()
    bf = od.best_f(models, Xm, des)
    seed = _next_sampler_seed(5)
    acq = rec.acquisition_values(exp.iloc[:60], space, obj, meas).to_numpy()
    want = od.model_scores(models, Xc[:60], None, des, "qLogEI", od.base_samples(512, 1, 2, seed), bf)
    dev_acq = float(np.abs(acq - want).max())
    seed = _next_sampler_seed(6)
    jv = rec.joint_acquisition_value(exp.iloc[[3, 140, 77]], space, obj, meas)
    rows = Xc[[3, 140, 77]]
    want_j = od.model_scores(models, rows[:1], rows[1:], des, "qLogEI", od.base_samples(512, 3, 2, seed), bf)[0]
    _record(f"recommender[{scalarizer},acquisition_values]", dev_acq, SCORE_ATOL)
    _record(f"recommender[{scalarizer},joint_acquisition_value]", abs(jv - want_j), SCORE_ATOL)
    assert dev_acq <= SCORE_ATOL and abs(jv - want_j) <= SCORE_ATOL
    with pytest.raises(IncompatibilityError, match="exceeds 16"):
        rec.recommend(17, space, obj, meas)
