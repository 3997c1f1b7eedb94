"""The objective-program kernels of baybe_amd/csrc/bbh_objacq.hip on the device, against tests/_oracle_objective.py.

  q = 1      ``bbh_mc_acq_obj_q1``: N = 1 and 257, S = 1, 33 and 512, every MC kind under six programs, rows that need the 1 x 1
             jitter, one masked row
  joint      ``bbh_mc_acq_obj_pending``: the synthetic joint statistics of tests/_joint_cases.py (p = 1, 2, 15; S = 33, 128; 130
             rows with every regime of its CYCLE; one single row), every kind under every program; NaN exactly on the rows that do
             not factor, -inf exactly on the masked rows
  identity   the programs [AFFINE(1, 0)] and [AFFINE(-1, 0)] reproduce ``bbh_mc_acq_q1`` / ``bbh_mc_acq_pending`` with sign = +1 / -1
  end to end ``HipBotorchRecommender`` with a bell target and a minimised absolute-value target: picks, acquisition values

Bounds: qLogEI ``_joint_cases.SCORE_ATOL``; the other kinds MC_RTOL / MC_ATOL of tests/test_joint_batch_gpu.py.  The inputs are
guarded by tests/test_objective_cpu.py::test_gpu_cases_do_not_depend_on_who_factored."""

import numpy as np
import pytest

import _objective_cases as oc
from _joint_cases import SCORE_ATOL, compare

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


def _program(ops):
    from baybe_amd.objective import ObjectiveProgram

    return ObjectiveProgram(tuple(ops))


def _record(name, value, tol):
    from conftest import record_deviation

    print(f"{name}: observed {value:.3e} (tolerance {tol:.1e})")
    record_deviation(f"objective/{name}", value, tol)


def _deviation(kind, got, ref):
    """(deviation in units of the kind's tolerance, tolerance as recorded)."""
    if kind == "qLogEI":
        return (float(np.abs(got - ref).max()) if len(ref) else 0.0), SCORE_ATOL
    return oc.mc_ratio(got, ref), 1.0


@pytest.mark.parametrize("N,S", oc.Q1_SHAPES, ids=[f"N{n}-S{s}" for n, s in oc.Q1_SHAPES])
def test_q1_every_kind_and_program(gp, N, S):
    import _oracle_objective as oo

    mean, var, z, alive = oc.q1_inputs(N, S)
    live = alive.astype(bool)
    dm, dv, da = _dev(mean), _dev(var), _dev(alive)
    failures = []
    worst = {k: 0.0 for k in oc.MC_KINDS}
    for pname, ops in oc.PROGRAMS.items():
        bf = oc.case_best_f(ops, mean)
        for kind in oc.MC_KINDS:
            got = gp.mc_acq(kind, dm, dv, z, bf, beta=oc.BETA, alive=da, objective=_program(ops)).cpu().numpy()
            ref = oo.q1_scores(kind, ops, mean, var, z, bf, oc.BETA)
            assert np.isfinite(ref[live]).all(), (pname, kind)
            if not (np.isneginf(got[~live]).all() and np.isfinite(got[live]).all()):
                failures.append((pname, kind, "masked / non-finite rows"))
                continue
            dev, tol = _deviation(kind, got[live], ref[live])
            worst[kind] = max(worst[kind], dev)
            if not dev <= tol:
                failures.append((pname, kind, dev))
    for kind in oc.MC_KINDS:
        _record(f"q1[N={N},S={S},{kind}]", worst[kind], SCORE_ATOL if kind == "qLogEI" else 1.0)
    assert not failures, failures


@pytest.mark.parametrize("case", oc.JOINT_CASES, ids=[c.id for c in oc.JOINT_CASES])
def test_joint_every_kind_and_program(gp, case):
    import _oracle_objective as oo

    d = case.build()
    Sig, means = oo.case_sigma(d)
    L = oo.lapack_factors(Sig)
    dm, dv, dc, da = _dev(d.mean), _dev(d.var), _dev(d.cross), _dev(d.alive)
    failures = []
    worst = {k: 0.0 for k in oc.MC_KINDS}
    for pname, ops in oc.PROGRAMS.items():
        bf = oc.case_best_f(ops, d.mean)
        for kind in oc.MC_KINDS:
            got = gp.mc_acq(kind, dm, dv, d.z, bf, beta=oc.BETA, alive=da, cross=dc, objective=_program(ops),
                            stats=(d.mean_p, d.cov_pp)).cpu().numpy()
            ref = np.where(d.alive.astype(bool), oo.scores_from_factors(kind, ops, means, L, d.z, bf, oc.BETA), -np.inf)
            if kind == "qLogEI":
                dev, tol = compare(got, case, ref), SCORE_ATOL  # NaN = notpd rows, -inf = masked rows, |difference| elsewhere
            else:
                compare(got, case, ref)  # (the row conventions)
                dev, tol = _deviation(kind, got[d.scored], ref[d.scored])
            worst[kind] = max(worst[kind], dev)
            if not dev <= tol:
                failures.append((pname, kind, dev))
    for kind in oc.MC_KINDS:
        _record(f"joint[{case.id},{kind}]", worst[kind], SCORE_ATOL if kind == "qLogEI" else 1.0)
    assert not failures, failures


# ---- agreement with the kernels of the untransformed path ---------------------------------------------------------------------
AGREE_D, AGREE_N_TRAIN, AGREE_CANDIDATES = 3, 20, 130


@pytest.fixture(scope="module")
def model(gp):
    from _problems import fixed_theta, make_problem
    from baybe_amd import gp_spec

    d = AGREE_D
    X, Xt, y = make_problem(2000, d, AGREE_N_TRAIN, seed=11)
    rows = np.unique(X, axis=0)  # distinct rows: a candidate never coincides with a pending point
    rows = rows[np.random.default_rng(3).permutation(len(rows))]
    pool, cand = rows[:15], np.ascontiguousarray(rows[15:15 + AGREE_CANDIDATES])
    ls, nz, _ = fixed_theta(d)
    gp.set_model(gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), Xt, y)
    gp.factorize(gp_spec.GPParams(np.full(d, ls), nz, 0.02))
    return pool, cand


@pytest.mark.parametrize("p", [0, 1, 4, 15], ids=lambda p: f"q{p + 1}")
def test_identity_and_negation_reproduce_the_sign_path(gp, model, p):
    from oracle import gp_oracle as go

    pool, cand = model
    z = go.sobol_normal_base_samples(64, p + 1, 3)
    stats = gp.set_pending(pool[:p]) if p else None
    mean, var = gp.posterior(cand)
    cross = gp.cross_cov(cand) if p else None
    failures = []
    worst = {k: 0.0 for k in oc.MC_KINDS}
    for sign in (1.0, -1.0):
        bf = gp.best_f(sign)
        prog = _program((("AFFINE", (sign, 0.0)),))
        assert bf == gp.best_f(1.0, prog)
        for kind in oc.MC_KINDS:
            zz = z[:, 0] if p == 0 else z
            old = gp.mc_acq(kind, mean, var, zz, bf, sign, beta=oc.BETA, cross=cross).cpu().numpy()
            new = gp.mc_acq(kind, mean, var, zz, bf, beta=oc.BETA, cross=cross, objective=prog, stats=stats).cpu().numpy()
            assert np.isfinite(old).all() and np.isfinite(new).all(), (kind, sign)
            dev, tol = _deviation(kind, new, old)
            worst[kind] = max(worst[kind], dev)
            if not dev <= tol:
                failures.append((kind, sign, dev))
    gp.set_pending(None)
    for kind in oc.MC_KINDS:
        _record(f"identity[q'={p + 1},{kind}]", worst[kind], SCORE_ATOL if kind == "qLogEI" else 1.0)
    assert not failures, failures


# ---- through the recommender ---------------------------------------------------------------------------------------------------
def _next_sampler_seed(seed_value):
    import torch

    torch.manual_seed(seed_value)
    s = int(torch.randint(0, 1000000, (1,)).item())
    torch.manual_seed(seed_value)
    return s


@pytest.mark.parametrize("which", ["match_bell", "match_absolute-min"])
def test_recommender_end_to_end(which):
    """n = 24, d = 3, 500 candidates: the picks are the oracle's greedy picks under the device's fitted hyper-parameters; the
    read-backs match; 17 points in one batch are refused."""
    import _oracle_objective as oo
    from _baybe_shim import NumericalDiscreteParameter, SearchSpace, SingleTargetObjective
    from baybe_amd.exceptions import IncompatibilityError
    from baybe_amd.objective import objective_program
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go

    rng = np.random.default_rng(8)
    space = SearchSpace.from_product([NumericalDiscreteParameter("x0", np.arange(10) / 9.0), NumericalDiscreteParameter("x1", np.arange(10) / 9.0),
                                      NumericalDiscreteParameter("x2", np.arange(5) / 4.0)])
    exp = space.discrete.exp_rep
    assert len(exp) == 500
    meas = exp.iloc[rng.choice(len(exp), 24, replace=False)].copy()
    Xm = meas[["x0", "x1", "x2"]].to_numpy(float)
    meas["y"] = Xm.sum(1) - 0.8 + 0.3 * np.sin(3 * Xm[:, 0]) + 0.02 * rng.standard_normal(len(Xm))
    target = oc.bell_target("y", 0.4, 0.3) if which == "match_bell" else oc.absolute_target("y", 0.7)
    ops = objective_program(target).ops
    obj = SingleTargetObjective(target)
    rec = HipBotorchRecommender()
    seed = _next_sampler_seed(1337)
    got = rec.recommend(3, space, obj, meas)
    prm = rec._surrogate_model.engine.params
    om = go.GPModel(go.GPSpec.baybe_default(3, np.zeros(3), np.ones(3)), go.GPParams(prm.lengthscale, prm.noise, prm.mean), Xm,
                    meas["y"].to_numpy())
    Xc = exp.to_numpy(float)
    idx, vals = oo.greedy(om, Xc, 3, seed, ops)
    assert got.index.tolist() == exp.index[idx].tolist()
    bf = oo.best_f(om, ops)
    seed = _next_sampler_seed(5)
    acq = rec.acquisition_values(exp.iloc[:60], space, obj, meas).to_numpy()
    want = oo.model_scores(om, Xc[:60], None, ops, "qLogEI", go.sobol_normal_base_samples(512, 1, seed), bf)
    dev_acq = float(np.abs(acq - want).max())
    seed = _next_sampler_seed(6)
    jv = rec.joint_acquisition_value(exp.iloc[[3, 140, 377]], space, obj, meas)
    rows = Xc[[3, 140, 377]]
    want_j = oo.model_scores(om, rows[:1], rows[1:], ops, "qLogEI", go.sobol_normal_base_samples(512, 3, seed), bf)[0]
    _record(f"recommender[{which},acquisition_values]", dev_acq, SCORE_ATOL)
    _record(f"recommender[{which},joint_acquisition_value]", abs(jv - want_j), SCORE_ATOL)
    assert dev_acq <= SCORE_ATOL and abs(jv - want_j) <= SCORE_ATOL
    with pytest.raises(IncompatibilityError, match="exceeds 16"):
        rec.recommend(17, space, obj, meas)
