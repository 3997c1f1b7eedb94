"""``bbh_polytope_sample`` / ``bbh_polytope_project`` and the recommender's linear-constraint path under
``continuous_optimizer="gradient"``, against the numpy / scipy statements of tests/_oracle_polytope.py.

Bounds
  * sampler: equal to the numpy restatement bit for bit; moments of the uniform simplex within 6 standard errors (the step count
    was chosen at 4, KERNELS.md 4.17).
  * projection, feasibility: the output is in [lo, hi] bit-exactly and |E x - e|_i, (g - G x)_i^+ <= C (dc + M) eps S_abs,i with
    S_abs,i = sum_k |row_ik x_k| + |rhs_i|, M = 2 dc + mi, C = ``POLY_C``.
  * projection, optimality: |x - x_exact|_inf <= 1e-12 max(1, |p|_inf) where the enumeration oracle applies (dc <= 4), the KKT
    residual (nnls) <= 1e-10 elsewhere.
"""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import _oracle_polytope as op
from conftest import record_deviation

pytestmark = pytest.mark.gpu

# C of the feasibility bound.  4 is the constant tests/test_continuous_gpu.py starts from (POSTGRAD_C) and the one the kernel is
# built with (BBH_POLY_FEAS_C): the projection refines its point until the bound holds with it, so the observed ratio is at most 1
# by construction (observed up to 0.93 on the fixtures below: it stops refining once the bound holds); no fixture needed more.
POLY_C = 4.0
DIST_RTOL = 1e-12
KKT_TOL = 1e-10


@pytest.fixture(scope="module")
def gp():
    from baybe_amd import engine

    g = engine.HipGP(0)
    g.selftest()
    yield g
    g.close()


def _np(t):
    return t.cpu().numpy()


def _poly(s):
    from baybe_amd.polytope import Polytope

    return Polytope(*s)


def _project(gp, P, X):
    R, t = P.rows()
    mu_min = 1e-10 * float((R * R).sum(axis=1).max()) if len(R) else 1.0
    tolf = POLY_C * (P.dc + P.n_rows) * op.EPS
    out, status = gp.polytope_project(np.ascontiguousarray(X, dtype=np.float64), P.lo, P.hi, R, t, P.me, tolf, mu_min)
    return _np(out), _np(status)


def _reduced_args(P):
    r = P.reduced()
    return r["Z"], r["GZ"], r["c0"], r["lo"], r["hi"], r["bl"], r["bu"], r["bg"]


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
# dc in {1, 2, 5, 32}, (me, mi) in {(0,1), (1,0), (1,3), (2,14)}, R in {1, 63, 64, 65, 257}, T in {1, 2, 33}: every value at least twice
SAMPLE_CASES = [
    (1, 0, 1, 1, 33), (1, 0, 1, 64, 2), (2, 1, 0, 63, 1), (2, 1, 3, 65, 33), (5, 2, 14, 257, 2),
    (5, 1, 0, 64, 1), (32, 2, 14, 63, 33), (32, 1, 3, 257, 1), (5, 0, 1, 65, 2), (32, 1, 0, 1, 2),
]


@pytest.mark.parametrize("dc,me,mi,R,T", SAMPLE_CASES)
def test_sampler_equals_the_numpy_restatement_bit_for_bit(gp, dc, me, mi, R, T):
    P = _poly(op.random_set(dc, me, mi, seed=1000 + 37 * dc + 5 * me + mi))
    seed = 0xC0FFEE0000000000 + R * 1000 + T  # (the upper half of the 64 bits is used too)
    got = _np(gp.polytope_sample(P.reduced(), R, T, seed))
    want = op.sample_oracle_reduced(*_reduced_args(P), R, T, seed)
    assert got.shape == (R, dc)
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert len(np.unique(got, axis=0)) == R  # (distinct chains)


def test_sampler_rows_do_not_depend_on_the_size_of_the_call(gp):
    P = _poly(op.random_set(5, 1, 3, seed=4))
    a = _np(gp.polytope_sample(P.reduced(), 257, 17, 99))
    b = _np(gp.polytope_sample(P.reduced(), 1000, 17, 99))
    c = _np(gp.polytope_sample(P.reduced(), 257, 17, 99))
    assert np.array_equal(a, b[:257]) and np.array_equal(a, c)
    assert not np.array_equal(a, _np(gp.polytope_sample(P.reduced(), 257, 17, 100)))


@pytest.mark.parametrize("dc", [4, 16])
def test_sampler_reproduces_the_moments_of_the_uniform_simplex(gp, dc):
    from baybe_amd.polytope import default_n_steps

    P = _poly(op.simplex(dc))
    T = default_n_steps(P.dz)
    X = _np(P.sample(gp, 4096, seed=20261021))
    z_mean, z_var = op.moment_z_scores(X, dc)
    worst = max(np.abs(z_mean).max(), np.abs(z_var).max())
    print(f"dc = {dc}, T = {T}: max |z| of the means {np.abs(z_mean).max():.2f}, of the variances {np.abs(z_var).max():.2f}")
    record_deviation(f"polytope_sampler_moments_z[dc={dc}]", worst, 6.0)
    assert worst <= 6.0
    ratio = op.feasibility_ratio(X, *op.simplex(dc), POLY_C).max()
    record_deviation(f"polytope_sampler_feasibility[dc={dc}]", ratio, 1.0)
    assert ratio <= 1.0


def test_public_sampler_takes_botorchs_arguments(gp):
    from baybe_amd.polytope import Polytope
    from baybe_amd.sampling import polytope_samples

    bounds = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    eq = [(np.array([0, 1, 2]), np.array([1.0, 1.0, 1.0]), 1.0)]
    ineq = [(np.array([0]), np.array([-1.0]), -0.6)]
    X = polytope_samples(bounds, eq, ineq, n=65, seed=5)
    P = Polytope.from_botorch(bounds, eq, ineq)
    assert X.shape == (65, 3) and np.array_equal(X, _np(P.sample(gp, 65, seed=5)))
    assert op.feasibility_ratio(X, P.lo, P.hi, P.E, P.e, P.G, P.g, POLY_C).max() <= 1.0
    pinned = polytope_samples(bounds, eq + [(np.array([0]), np.array([1.0]), 0.2), (np.array([1]), np.array([1.0]), 0.3)], None, n=4, seed=1)
    assert np.allclose(pinned, [[0.2, 0.3, 0.5]] * 4, atol=1e-15)


# ---- projection against the enumeration oracle --------------------------------------------------------------------------------------
def _small_sets():
    """dc = 1, 2, 2 (with an equality), 4: each carries a duplicated inequality row and a vertex with more active rows than dz."""
    z = np.zeros
    return {
        "dc1": ((z(1), np.ones(1), z((0, 1)), z(0), np.array([[1.0], [1.0]]), np.array([0.2, 0.2])),
                np.array([[0.5], [0.2], [1.0], [0.1], [-7.0], [30.0], [1.0 + 1e-9]])),
        "dc2": ((z(2), np.ones(2), z((0, 2)), z(0), np.array([[1.0, 1.0], [1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]]), np.array([0.5, 0.5, -1.5, -1.0])),
                np.array([[0.5, 0.5], [0.25, 0.25], [0.0, 1.0], [-0.3, 1.4], [0.1, 0.1], [20.0, -30.0], [-15.0, 40.0], [0.5, 1.0], [0.7, 0.9]])),
        "dc2eq": ((z(2), np.ones(2), np.array([[1.0, 1.0]]), np.array([1.0]), np.array([[1.0, 0.0], [1.0, 0.0]]), np.array([0.2, 0.2])),
                  np.array([[0.5, 0.5], [0.2, 0.8], [1.0, 0.0], [0.0, 0.0], [-3.0, 0.5], [25.0, 31.0], [0.9, 0.9]])),
        "dc4": ((z(4), np.ones(4), np.ones((1, 4)), np.array([1.0]), np.array([[-1.0, 0, 0, 0], [-1.0, 0, 0, 0], [0, 1.0, 1.0, 0]]), np.array([-0.6, -0.6, 0.1])),
                np.array([[0.25, 0.25, 0.25, 0.25], [0.6, 0.2, 0.1, 0.1], [0.6, 0.4, 0.0, 0.0], [0.9, 0.5, -0.2, -0.2], [0.3, 0.05, 0.05, 0.6],
                          [12.0, -9.0, 3.0, 0.5], [-20.0, -20.0, -20.0, 50.0], [0.0, 0.0, 0.0, 1.0], [0.1, 0.2, 0.3, 0.4000001]])),
    }


@pytest.fixture(scope="module")
def exact_projections():
    """Computed once: {name: (set, points, exact projections)}."""
    return {name: (s, X, np.array([op.project_exact(x, *s) for x in X])) for name, (s, X) in _small_sets().items()}


@pytest.mark.parametrize("name", ["dc1", "dc2", "dc2eq", "dc4"])
def test_projection_against_the_enumeration_oracle(gp, exact_projections, name):
    s, X, want = exact_projections[name]
    P = _poly(s)
    got, status = _project(gp, P, X)
    assert (status == 0).all(), status
    err = np.abs(got - want).max(axis=1) / np.maximum(1.0, np.abs(X).max(axis=1))
    ratio = op.feasibility_ratio(got, *s, POLY_C).max()
    print(f"{name}: worst |x - x_exact| / max(1, |p|) = {err.max():.3e}, worst feasibility ratio {ratio:.3f}")
    record_deviation(f"polytope_project_exact[{name}]", float(err.max()), DIST_RTOL)
    assert err.max() <= DIST_RTOL, err
    assert ratio <= 1.0


# ---- projection at size -------------------------------------------------------------------------------------------------------------
def _inputs(P, k, seed):
    """k rows: the centre, points of the box (mostly outside the set), near the set (a tenth of the box away), far outside (three
    box widths away, every coordinate clipped at first) and corners of the box."""
    rng = np.random.default_rng(seed)
    span = P.hi - P.lo
    kinds = [P.c0[None, :],
             P.lo + span * rng.random((k, P.dc)),
             P.c0 + 0.1 * span * rng.normal(size=(k, P.dc)),
             P.c0 + 3.0 * span * rng.normal(size=(k, P.dc)),
             P.lo + span * rng.integers(0, 2, (k, P.dc))]
    pick = np.concatenate([[0], 1 + np.arange(k - 1) % 4]) if k > 1 else np.array([3])
    return np.array([kinds[j][i if j else 0] for i, j in enumerate(pick)])


PROJECT_CASES = [(5, 1, 0, 1), (5, 1, 3, 63), (5, 2, 14, 65), (5, 0, 16, 257), (32, 1, 0, 257), (32, 1, 3, 65), (32, 2, 14, 63), (32, 0, 16, 1)]


@pytest.mark.parametrize("dc,me,mi,k", PROJECT_CASES)
def test_projection_meets_feasibility_and_kkt_at_size(gp, dc, me, mi, k):
    s = op.random_set(dc, me, mi, seed=7 + dc + mi)
    P = _poly(s)
    X = _inputs(P, k, seed=dc + k)
    got, status = _project(gp, P, X)
    assert got.shape == (k, dc) and (status == 0).all(), np.flatnonzero(status)
    ratio = op.feasibility_ratio(got, P.lo, P.hi, P.E, P.e, P.G, P.g, POLY_C).max()
    kkt = max(op.kkt_residual(p, x, P.lo, P.hi, P.E, P.e, P.G, P.g) for p, x in zip(X, got))
    print(f"dc={dc} me={me} mi={mi} k={k}: worst feasibility ratio {ratio:.3f}, worst KKT residual {kkt:.3e}")
    record_deviation(f"polytope_project_feasibility[dc={dc},me={me},mi={mi},k={k}]", ratio, 1.0)
    record_deviation(f"polytope_project_kkt[dc={dc},me={me},mi={mi},k={k}]", kkt, KKT_TOL)
    assert ratio <= 1.0
    assert kkt <= KKT_TOL


def test_projection_bitwise_properties(gp):
    s = op.random_set(32, 2, 14, seed=11)
    P = _poly(s)
    X = _inputs(P, 257, seed=3)
    X[[5, 20, 256]] = X[2]
    once, st1 = _project(gp, P, X)
    twice, st2 = _project(gp, P, once)
    again, _ = _project(gp, P, X)
    alone, st3 = _project(gp, P, X[2:3])
    assert (st1 == 0).all() and (st2 == 0).all() and st3[0] == 0
    assert np.array_equal(twice, once)  # a feasible row comes back bit for bit: a frozen start does not drift
    assert np.array_equal(again, once)  # two runs
    for r in (5, 20, 256):
        assert np.array_equal(once[r], once[2])  # equal rows, wherever they stand
    assert np.array_equal(alone[0], once[2])  # whatever k is
    inside = P.c0[None, :] + 0.0
    assert np.array_equal(_project(gp, P, once[:7])[0], once[:7]) and _project(gp, P, inside)[1][0] == 0
    assert (once >= P.lo).all() and (once <= P.hi).all()


def test_projection_names_bad_arguments(gp):
    from baybe_amd._lib import HipError

    P = _poly(op.simplex(3))
    R, t = P.rows()
    with pytest.raises(HipError, match="me \\+ mi <= 16 rows"):
        gp.polytope_project(np.zeros((2, 3)), P.lo, P.hi, np.ones((17, 3)), np.ones(17), 1, 1e-14, 1e-10)
    with pytest.raises(HipError, match="lo <= hi"):
        gp.polytope_project(np.zeros((2, 3)), P.hi, P.lo, R, t, 1, 1e-14, 1e-10)
    out, status = gp.polytope_project(np.array([[np.nan, 0.2, 0.3]]), P.lo, P.hi, R, t, 1, 1e-14, 1e-10)
    assert _np(status)[0] == 1 and np.isfinite(_np(out)).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _objective():
    return SimpleNamespace(targets=(SimpleNamespace(name="y", minimize=False, transformation=None),), is_multi_output=False)


def _con(parameters, operator, coefficients, rhs, interpoint=False):
    return SimpleNamespace(parameters=list(parameters), operator=operator, coefficients=tuple(coefficients), rhs=rhs, is_interpoint=interpoint)


def _space(hybrid: bool, eq=None, ineq=None):
    from _replay import HybridSpace

    disc = pd.DataFrame({"d0": [0.25, 0.75], "d1": [0.5, 0.25]}) if hybrid else pd.DataFrame()
    bounds = pd.DataFrame([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], index=["min", "max"], columns=["c0", "c1", "c2"])
    space = HybridSpace(disc, bounds)
    space.continuous.constraints_lin_eq = tuple(eq if eq is not None else [_con(["c0", "c1", "c2"], "=", [1.0, 1.0, 1.0], 1.0)])
    space.continuous.constraints_lin_ineq = tuple(ineq if ineq is not None else [_con(["c0"], "<=", [1.0], 0.6)])
    return space, disc


def _measurements(space, hybrid: bool):
    """The training data of ``make_case`` (2 discrete + 3 continuous columns), mapped from its box to the unit box."""
    from _continuous_cases import make_case

    _, _, Xt, y, lo, hi = make_case("matern52", True, 24, 3, seed=21)
    U = (Xt - lo) / (hi - lo)
    if hybrid:
        U[:, :2] = np.array([[0.25, 0.5], [0.75, 0.25]])[np.arange(len(U)) % 2]
    else:
        U = U[:, 2:]
    return pd.DataFrame(U, columns=list(space.comp_rep_columns)).assign(y=y)


@pytest.mark.parametrize("hybrid", [False, True])
def test_constrained_recommendation_is_feasible_and_reaches_the_dense_feasible_grid(hybrid):
    """3 columns in [0, 1] with c0 + c1 + c2 = 1 and c0 <= 0.6 (continuous, and behind 2 discrete rows): every returned point meets
    the feasibility bound; the first point's qLogEI on the oracle is at least the maximum over a dense feasible grid - 1e-3 (the
    margin of tests/test_hybrid_cpu.py against its dense grid); the second point is another point; the trace counts projections.
    Without the feature this raises the "box-bounded" IncompatibilityError."""
    import torch

    from _continuous_cases import oracle_model
    from baybe_amd import engine
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go
    from oracle import hybrid_oracle as ho

    space, disc = _space(hybrid)
    meas = _measurements(space, hybrid)
    rec = HipBotorchRecommender(continuous_optimizer="gradient")
    torch.manual_seed(7)
    got = rec.recommend(2, space, _objective(), meas)
    torch.manual_seed(7)
    engine.draw_sampler_seed()  # (the raw samples' seed)
    seed = engine.draw_sampler_seed()  # the acquisition function's sampler seed of that call
    picks = got.to_numpy(dtype=float)
    dd = disc.shape[1]
    assert picks.shape == (2, dd + 3) and list(got.columns) == list(space.comp_rep_columns)
    lo, hi, E, e, G, g = np.zeros(3), np.ones(3), np.ones((1, 3)), np.ones(1), np.array([[-1.0, 0.0, 0.0]]), np.array([-0.6])
    ratio = op.feasibility_ratio(picks[:, dd:], lo, hi, E, e, G, g, POLY_C).max()
    record_deviation(f"polytope_recommendation_feasibility[{'hybrid' if hybrid else 'cont'}]", ratio, 1.0)
    assert ratio <= 1.0, ratio
    eng = rec._surrogate_model.engine
    om = oracle_model(eng.spec, eng.params, eng._X_train, eng._y_train)
    best_f = go.best_f_from_model(om)
    z = go.sobol_normal_base_samples(512, 1, seed)
    n = 80
    grid = np.array([[a / n, b / n, (n - a - b) / n] for a in range(0, int(0.6 * n) + 1) for b in range(0, n - a + 1)])
    D = disc.to_numpy(dtype=float) if hybrid else np.zeros((1, 0))
    dense = np.vstack([np.hstack([np.tile(row, (len(grid), 1)), grid]) for row in D])
    none = np.zeros((0, dd + 3))
    v_grid = ho._scores(om, dense, none, z, best_f, 1.0).max()
    v_first = float(ho._scores(om, picks[:1], none, z, best_f, 1.0)[0])
    tr = rec._last_continuous_trace
    print(f"hybrid {hybrid}: first point {v_first:.9f}, dense feasible grid {v_grid:.9f}; {len(tr[0]['starts'])} starts, "
          f"{tr[0]['calls']} device passes, {tr[0]['projections']} projection calls")
    record_deviation(f"polytope_recommendation_grid_gap[{'hybrid' if hybrid else 'cont'}]", max(v_grid - v_first, 0.0), 1e-3)
    assert v_first >= v_grid - 1e-3, (v_first, v_grid)
    assert np.linalg.norm(picks[0] - picks[1]) > 1e-3
    assert len(tr) == 2 and all(step["projections"] >= 1 for step in tr)
    if hybrid:
        assert all((row[:dd] == D).all(axis=1).any() for row in picks)


def test_refusals_reach_the_user_before_any_fit(monkeypatch):
    from baybe_amd.exceptions import IncompatibilityError
    from baybe_amd.recommenders import HipBotorchRecommender, HipRecommenderImpl

    def no_fit(*a, **k):
        raise AssertionError("the surrogate was fitted before the refusal")

    monkeypatch.setattr(HipRecommenderImpl, "get_surrogate", no_fit)
    rng = np.random.default_rng(0)
    many = [_con(["c0", "c1", "c2"], ">=", rng.normal(size=3), -5.0) for _ in range(16)]
    cases = [(dict(ineq=many), "17 linear constraint rows"),
             (dict(ineq=[_con(["c0"], "<=", [1.0], 0.6, interpoint=True)]), "Interpoint"),
             (dict(ineq=[_con(["c0", "c1"], ">=", [1.0, 1.0], 2.5)]), "no feasible point")]
    for kw, text in cases:
        space, _ = _space(False, **kw)
        meas = _measurements(space, False)
        with pytest.raises(IncompatibilityError, match=text):
            HipBotorchRecommender(continuous_optimizer="gradient").recommend(1, space, _objective(), meas)
        with pytest.raises(IncompatibilityError, match="box-bounded"):
            HipBotorchRecommender().recommend(1, space, _objective(), meas)
