"""Device-side derivatives for gradient-based continuous refinement: ``bbh_posterior_grad``, ``bbh_qlogei_partials``, their
composition and the recommender's ``continuous_optimizer="gradient"`` path, against the numpy oracle.

Bounds
  * posterior derivatives, entry-wise: |dev - oracle| <= C (n + 16) eps S_abs, S_abs = the sum of the absolute values of the
    entry's terms as the oracle forms them (tests/_oracle_continuous.py); C as recorded next to ``POSTGRAD_C`` below.
  * values from the same call: the tolerances tests/test_gpu_parity.py applies to ``bbh_posterior`` / ``bbh_cross_cov``.
  * derivatives against finite differences: the two-step criterion |g - FD_{h/2}| <= |FD_h - FD_{h/2}| + 16 eps |f| / h.
"""

import numpy as np
import pytest

from _continuous_cases import make_case, oracle_model, random_rows
from _oracle_continuous import EPS, posterior_grad_oracle, two_step_ok
from conftest import record_deviation

pytestmark = pytest.mark.gpu

MEAN_RTOL, VAR_RTOL, SCORE_ATOL = 1e-9, 1e-8, 1e-8  # tests/test_gpu_parity.py
# C of the posterior-derivative bound.  4 is the linear surrogate's constant (tests/test_linear_gpu.py) and holds for d mean and
# d cross (observed <= 0.11 of it).  d var carries w = (K + s2 I)^-1 k*, which the device takes from the explicit inverse X^T X and the
# oracle from two triangular solves: either errs by up to cond(K + s2 I) eps |w|, which (n + 16) eps does not cover at small n
# (observed 1.73 of the bound with C = 4 at n = 17, d = 35; <= 0.7 elsewhere) - hence 16 for that output alone (KERNELS.md 4.12).
POSTGRAD_C = {"dmean": 4.0, "dcross": 4.0, "dvar": 16.0}


@pytest.fixture(scope="module")
def gp():
    from baybe_amd import engine

    g = engine.HipGP(0)
    g.selftest()
    yield g
    g.close()


def _np(t):
    return t.cpu().numpy()


# kernel kind x outputscale, n in {1, 16, 17, 511, 512}, N in {1, 17, 33}, dc in {1, 5, 32}, p in {0, 1, 15}: every value of every
# axis at least twice, the large sizes with every kernel kind
POSTGRAD_CASES = [
    ("matern52", True, 512, 33, 32, 15), ("matern32", False, 511, 17, 5, 1), ("rbf", True, 512, 1, 1, 0),
    ("matern52", False, 17, 17, 32, 0), ("matern32", True, 16, 33, 1, 15), ("rbf", False, 1, 1, 5, 1),
    ("matern52", True, 1, 33, 1, 1), ("matern32", False, 512, 33, 5, 0), ("rbf", True, 511, 17, 32, 15),
    ("matern52", False, 16, 1, 5, 15), ("matern32", True, 17, 1, 32, 1), ("rbf", False, 16, 17, 1, 0),
    ("matern52", False, 511, 33, 1, 1), ("matern32", True, 512, 17, 32, 15), ("rbf", False, 17, 33, 5, 15),
]


@pytest.mark.parametrize("kernel,use_os,n,N,dc,p", POSTGRAD_CASES)
def test_posterior_grad_against_the_closed_form_oracle(gp, kernel, use_os, n, N, dc, p):
    d_cont = dc + 1
    spec, prm, Xt, y, lo, hi = make_case(kernel, use_os, n, d_cont, seed=100 + n + dc)
    cols = [c for c in range(2, 2 + d_cont) if c != (3 if d_cont > 1 else -1)]  # skips one continuous column
    assert len(cols) == dc
    om = oracle_model(spec, prm, Xt, y)
    X = random_rows(lo, hi, N, seed=7)
    X[0] = Xt[0]  # a row equal to a training point
    pend = random_rows(lo, hi, p, seed=8) if p else None
    gp.set_model(spec, Xt, y)
    gp.factorize(prm)
    gp.set_pending(pend)
    out = {k: _np(v) for k, v in gp.posterior_grad(X, cols).items()}
    ref = posterior_grad_oracle(om, X, cols, pend)
    worst = 0.0
    for key in ("dmean", "dvar") + (("dcross",) if p else ()):
        bound = POSTGRAD_C[key] * (n + 16) * EPS * ref["S_" + key]
        err = np.abs(out[key] - ref[key])
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print(f"{key}: worst |dev - oracle| / bound = {ratio:.3f}  (max |entry| {np.abs(ref[key]).max():.3e})")
    record_deviation(f"posterior_grad[{kernel},{int(use_os)},n={n},N={N},dc={dc},p={p}]", worst, 1.0)
    # the values of the same call against the two value calls, at the tolerances of tests/test_gpu_parity.py
    m, v = gp.posterior(X)
    assert np.allclose(out["mean"], _np(m), rtol=MEAN_RTOL, atol=1e-12)
    assert np.allclose(out["var"], _np(v), rtol=VAR_RTOL, atol=1e-14)
    if p:
        assert np.allclose(out["cross"], _np(gp.cross_cov(X)), rtol=1e-7, atol=1e-12)
    gp.set_pending(None)
    assert worst <= 1.0, worst


def test_posterior_grad_gives_equal_rows_equal_bits(gp):
    spec, prm, Xt, y, lo, hi = make_case("matern52", True, 40, 5, seed=3)
    gp.set_model(spec, Xt, y)
    gp.factorize(prm)
    gp.set_pending(random_rows(lo, hi, 2, seed=5))
    X = random_rows(lo, hi, 37, seed=6)
    X[[5, 20, 36]] = X[2]
    a = {k: _np(v) for k, v in gp.posterior_grad(X, [2, 3, 5]).items()}
    b = {k: _np(v) for k, v in gp.posterior_grad(X[2:3], [2, 3, 5]).items()}
    gp.set_pending(None)
    for key in a:
        for r in (5, 20, 36):
            assert np.array_equal(a[key][r], a[key][2]), key
        assert np.array_equal(a[key][2], b[key][0]), key


def test_posterior_grad_names_the_unmet_condition(gp):
    from baybe_amd import gp_spec
    from baybe_amd._lib import HipError

    spec, prm, Xt, y, lo, hi = make_case("matern52", False, 20, 3, seed=2)
    gp.set_model(spec, Xt, y)
    gp.factorize(prm)
    X = random_rows(lo, hi, 4, seed=1)
    with pytest.raises(HipError, match="ascending numerical columns"):
        gp.posterior_grad(X, [3, 2])
    with pytest.raises(HipError, match="1 <= dc <= 32"):
        gp.posterior_grad(X, [])
    spec12 = gp_spec.GPSpec.baybe_default(5, lo, hi, kernel="matern12")
    gp.set_model(spec12, Xt, y)
    gp.factorize(gp_spec.GPParams(np.full(5, 0.5), 0.02, 0.0))
    with pytest.raises(HipError, match="Matern-3/2, Matern-5/2 or RBF"):
        gp.posterior_grad(X, [2])


# ---- qLogEI partials ---------------------------------------------------------------------------------------------------
def _joint_score(go, m0, v0, c, mp, cpp, z, bf, sign):
    if len(mp) == 0:
        return float(go.qlogei_q1(np.array([m0]), np.array([v0]), z[:, 0], bf, sign)[0])
    cov = np.empty((1 + len(mp), 1 + len(mp)))
    cov[0, 0], cov[0, 1:], cov[1:, 0], cov[1:, 1:] = v0, c, c, cpp
    return go.qlogei_joint(np.concatenate([[m0], mp]), cov, z, bf, sign)


@pytest.mark.parametrize("p", [0, 1, 3, 15])
@pytest.mark.parametrize("S", [1, 8, 13, 512])
def test_qlogei_partials_against_the_oracle_and_its_differences(gp, p, S):
    from oracle import gp_oracle as go

    N = 65 if (p + S) % 2 == 0 else 1
    sign = -1.0 if p == 3 else 1.0
    spec, prm, Xt, y, lo, hi = make_case("matern52", True, 24, 6, seed=3)
    om = oracle_model(spec, prm, Xt, y)
    gp.set_model(spec, Xt, y)
    gp.factorize(prm)
    pend = random_rows(lo, hi, p, seed=11, spread=0.3) if p else None
    stats = gp.set_pending(pend)
    mp, cpp = (stats if p else (np.zeros(0), np.zeros((0, 0))))
    X = random_rows(lo, hi, N + 2, seed=9, spread=0.3)
    g = gp.posterior_grad(X, [2, 3, 4, 5, 6, 7])
    mean, var, cross = g["mean"].clone(), g["var"].clone(), g["cross"].clone()
    var[N] = 0.0  # edge: no variance
    if p:  # edge: a copy of the first pending point
        mean[N + 1], var[N + 1] = float(mp[0]), float(cpp[0, 0])
        cross[N + 1] = cross.new_tensor(cpp[0])
    z = go.sobol_normal_base_samples(S, 1 + p, 5)
    bf = go.best_f_from_model(om, sign)
    scores, part, ok = (_np(t) for t in gp.qlogei_partials(mean, var, cross, z, bf, sign))
    if p:  # the edge rows: exactly as the value kernel scores them
        ref_edge = _np(gp.qlogei_pending(mean, var, cross, z, bf, sign))
        for e in (N, N + 1):
            assert ok[e] == 0 and not part[e].any()
            assert (np.isnan(scores[e]) and np.isnan(ref_edge[e])) or abs(scores[e] - ref_edge[e]) <= SCORE_ATOL
    else:
        assert ok[N] == 0 and not part[N].any() and np.isfinite(scores[N])
        assert ok[N + 1] == 1
    gp.set_pending(None)
    mh, vh, ch = _np(mean), _np(var), _np(cross)
    worst_s, worst_g = 0.0, 0.0
    for i in range(N):
        assert ok[i] == 1
        f = _joint_score(go, mh[i], vh[i], ch[i], mp, cpp, z, bf, sign)
        worst_s = max(worst_s, abs(scores[i] - f))
        # h scaled to the entry: the score depends on an entry through t = (sign y - best_f) / tau_relu, tau_relu = 1e-6, and a
        # sample near the improvement boundary bends over |delta y| ~ tau_relu - the step moves y by 1e-2 tau_relu for |z| ~ 1
        # (mean: delta y = h; var: delta y_0 = z h / (2 sd); cross_r: delta y_r = z_0 h / sd)
        sd = np.sqrt(vh[i])
        entries = [("mean", 1e-8), ("var", 2e-8 * sd)] + [(r, 1e-8 * sd) for r in range(p)]
        for k, (what, h) in enumerate(entries):
            def at(delta):
                m0, v0, c = mh[i], vh[i], ch[i].copy()
                if what == "mean":
                    m0 += delta
                elif what == "var":
                    v0 += delta
                else:
                    c[what] += delta
                return _joint_score(go, m0, v0, c, mp, cpp, z, bf, sign)
            x0 = mh[i] if what == "mean" else vh[i] if what == "var" else ch[i][what]

            def fd(step):  # over the step the perturbed entry actually takes (h is ~1e-8 of the entry: x0 + h rounds)
                return (at(step) - at(-step)) / ((x0 + step) - (x0 - step))

            fd_h, fd_h2 = fd(h), fd(h / 2)
            holds, err, bound = two_step_ok(part[i, k], fd_h, fd_h2, f, h)
            worst_g = max(worst_g, float(err / bound))
            assert holds, (i, what, part[i, k], fd_h, fd_h2, err, bound)
    print(f"p={p} S={S} N={N}: worst |score - oracle| {worst_s:.3e}, worst derivative error / bound {worst_g:.3f}")
    record_deviation(f"qlogei_partials_score[p={p},S={S}]", worst_s, SCORE_ATOL)
    assert worst_s <= SCORE_ATOL


# ---- composed gradient ---------------------------------------------------------------------------------------------------
def test_qlogei_value_grad_against_differences_of_the_oracle(gp):
    from oracle import gp_oracle as go

    spec, prm, Xt, y, lo, hi = make_case("matern52", True, 24, 6, seed=3)
    om = oracle_model(spec, prm, Xt, y)
    gp.set_model(spec, Xt, y)
    gp.factorize(prm)
    pend = random_rows(lo, hi, 3, seed=11, spread=0.3)
    gp.set_pending(pend)
    X = random_rows(lo, hi, 5, seed=9, spread=0.3)
    cols = [2, 3, 4, 5, 6, 7]
    z = go.sobol_normal_base_samples(64, 4, 5)
    bf = go.best_f_from_model(om, 1.0)
    scores, grad, ok = (_np(t) for t in gp.qlogei_value_grad(X, cols, z, bf, 1.0))
    gp.set_pending(None)
    assert ok.all()
    ref = go.qlogei_with_pending(om, X, pend, z, bf, 1.0)
    assert np.allclose(scores, ref, rtol=0, atol=SCORE_ATOL)
    h, worst = 1e-4, 0.0
    for i in range(len(X)):
        for k, c in enumerate(cols):
            def at(delta):
                x = X[i : i + 1].copy()
                x[0, c] += delta
                return go.qlogei_with_pending(om, x, pend, z, bf, 1.0)[0]
            fd_h = (at(h) - at(-h)) / (2 * h)
            fd_h2 = (at(h / 2) - at(-h / 2)) / h
            holds, err, bound = two_step_ok(grad[i, k], fd_h, fd_h2, ref[i], h)
            worst = max(worst, float(err / bound))
            assert holds, (i, c, grad[i, k], fd_h, fd_h2, err, bound)
    print(f"composed gradient: worst error / bound {worst:.3f}")


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _objective():
    from types import SimpleNamespace

    return SimpleNamespace(targets=(SimpleNamespace(name="y", minimize=False, transformation=None),), is_multi_output=False)


def _oracle_of(eng):
    from _problems import oracle_params, oracle_spec
    from oracle import gp_oracle as go

    return go.GPModel(oracle_spec(eng.spec), oracle_params(eng.spec, eng.params), eng._X_train, eng._y_train)


@pytest.mark.parametrize("dc,levels,q", [(2, 4, 3), (4, 2, 3)])
def test_gradient_picks_reach_the_enumeration_oracles_optimum(dc, levels, q):
    """The fixtures of tests/test_hybrid_gpu.py under ``continuous_optimizer="gradient"``: every step's value, scored by the oracle,
    is within 1e-6 of the enumeration oracle's optimum (the gap the compass search is held to); the discrete part is a row of the
    subspace, bit for bit."""
    import itertools

    import pandas as pd
    import torch

    from _replay import HybridSpace
    from baybe_amd import engine
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go
    from oracle import hybrid_oracle as ho

    rng = np.random.default_rng(10 + dc)
    lv = np.linspace(0, 1, levels)
    disc = pd.DataFrame(list(itertools.product(lv, lv)), columns=["d0", "d1"])
    cb = np.array([[0.0, -1.0, 0.5, 0.0][:dc], [1.0, 2.0, 1.5, 2.0][:dc]])
    bounds = pd.DataFrame(cb, index=["min", "max"], columns=[f"c{a}" for a in range(dc)])
    space = HybridSpace(disc, bounds)
    opt = np.array([0.3, 1.2, 0.9, 1.4][:dc])

    def truth(M):
        return -((M[:, :2] - 0.45) ** 2).sum(1) - (0.6 * (M[:, 2:] - opt) ** 2).sum(1) + 0.05 * np.sin(5.0 * M[:, 2])

    n = 18
    M = np.hstack([disc.to_numpy()[rng.choice(len(disc), n)], cb[0] + rng.random((n, dc)) * (cb[1] - cb[0])])
    meas = pd.DataFrame(M, columns=list(space.comp_rep_columns)).assign(y=truth(M))
    rec = HipBotorchRecommender(continuous_optimizer="gradient")
    torch.manual_seed(7)
    got = rec.recommend(q, space, _objective(), meas)
    torch.manual_seed(7)
    engine.draw_sampler_seed()  # (the raw samples' Sobol seed)
    seed = engine.draw_sampler_seed()  # the acquisition function's sampler seed of that call
    om = _oracle_of(rec._surrogate_model.engine)
    best_f = go.best_f_from_model(om)
    picks = got.to_numpy(dtype=float)
    D = disc.to_numpy(dtype=float)
    worst = 0.0
    for step in range(q):
        pend = picks[:step]
        z = go.sobol_normal_base_samples(512, 1 + step, seed)
        row, c_opt, v_opt, _ = ho.mixed_step(om, D, cb, pend, z, best_f)
        v_dev = float(ho._scores(om, picks[step : step + 1], pend, z, best_f, 1.0)[0])
        worst = max(worst, v_opt - v_dev)
        tr = rec._last_continuous_trace[step]
        print(f"d_c = {dc} step {step}: oracle {v_opt:.9f}, device {v_dev:.9f}; {len(tr['starts'])} starts, {tr['calls']} passes")
        assert v_opt - v_dev <= 1e-6, (dc, step, v_opt - v_dev)
        assert (picks[step, :2] == D).all(axis=1).any()
    record_deviation(f"gradient_enumeration_value_gap_dc{dc}", worst, 1e-6)


def _high_dimensional_run(dc: int, hybrid: bool):
    """One recommendation of q = 2 under "gradient" on the bowl -sum (x - 0.4)^2 plus small noise, n = 24: (recommender, picks,
    discrete rows, box, sampler seed)."""
    import pandas as pd
    import torch

    from _replay import HybridSpace
    from baybe_amd import engine
    from baybe_amd.acquisition import qLogExpectedImprovement
    from baybe_amd.recommenders import HipBotorchRecommender

    rng = np.random.default_rng(40 + dc)
    disc = pd.DataFrame({"d0": [0.0, 0.5, 1.0]}) if hybrid else pd.DataFrame()
    cb = np.vstack([np.zeros(dc), np.ones(dc)])
    bounds = pd.DataFrame(cb, index=["min", "max"], columns=[f"c{a}" for a in range(dc)])
    space = HybridSpace(disc, bounds)
    n = 24
    cols = [rng.choice([0.0, 0.5, 1.0], (n, 1))] if hybrid else []
    M = np.hstack(cols + [rng.random((n, dc))])
    meas = pd.DataFrame(M, columns=list(space.comp_rep_columns)).assign(y=-((M - 0.4) ** 2).sum(1) + 0.01 * rng.normal(size=n))
    rec = HipBotorchRecommender(continuous_optimizer="gradient", n_restarts=4,
                                acquisition_function=qLogExpectedImprovement(n_mc_samples=128))
    torch.manual_seed(11)
    got = rec.recommend(2, space, _objective(), meas)
    torch.manual_seed(11)
    engine.draw_sampler_seed()
    seed = engine.draw_sampler_seed()
    return rec, got.to_numpy(dtype=float), disc.to_numpy(dtype=float), cb, seed


@pytest.mark.parametrize("dc,hybrid", [(6, False), (6, True), (12, False), (12, True)])
def test_gradient_refinement_matches_scipy_on_the_oracle_beyond_four_dimensions(dc, hybrid):
    """d_c = 6 and 12, continuous-only and with 3 discrete rows.  Per step scipy's L-BFGS-B climbs the ORACLE's value (the options of
    ``hybrid_oracle.mixed_step``) from every start on ``_last_continuous_trace`` and once more from the device's final point: the
    device's best value is at least the best of those runs minus 1e-6, and the run from its own final point gains at most 1e-6 (the
    convergence check).  Only the best is held - a multi-start search promises its best; the share of starts on which the device
    ends more than 1e-6 below scipy is recorded.  Observed: the device's best equals scipy's best to the last printed digit (1e-9) in
    all eight steps, the polish gains at most 2e-15; scipy's runs from the starts of ONE row agree to 1e-14 in the first step, while
    starts of different rows and of the second step (the first pick pending) end in different basins (spread up to 3.8), which is why
    only the best is held; the device ends below scipy on 0 (d_c = 6) and 8 - 13 % (d_c = 12) of the starts."""
    import scipy.optimize as sopt

    from oracle import gp_oracle as go
    from oracle import hybrid_oracle as ho

    rec, picks, D, cb, seed = _high_dimensional_run(dc, hybrid)
    dd = D.shape[1]
    om = _oracle_of(rec._surrogate_model.engine)
    best_f = go.best_f_from_model(om)
    behind, total = 0, 0
    for step in range(2):
        pend = picks[:step]
        z = go.sobol_normal_base_samples(128, 1 + step, seed)
        tr = rec._last_continuous_trace[step]

        def climb(row):
            def neg(c):
                return -float(ho._scores(om, np.concatenate([row[:dd], c])[None, :], pend, z, best_f, 1.0)[0])

            res = sopt.minimize(neg, row[dd:], method="L-BFGS-B", bounds=list(zip(cb[0], cb[1])),
                                options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 200})
            return max(-float(res.fun), -neg(row[dd:]))

        v_dev = float(ho._scores(om, picks[step : step + 1], pend, z, best_f, 1.0)[0])
        runs = np.array([climb(s) for s in tr["starts"]])
        finals = ho._scores(om, tr["final"], pend, z, best_f, 1.0)
        behind += int((finals < runs - 1e-6).sum())
        total += len(runs)
        polish = climb(picks[step])
        print(f"d_c = {dc} hybrid {hybrid} step {step}: device {v_dev:.9f}, scipy best {runs.max():.9f} (spread {runs.max() - runs.min():.2e}), "
              f"polish gain {polish - v_dev:.2e}; {len(runs)} starts, {tr['calls']} device passes")
        assert np.array_equal(tr["final"][tr["best"]], picks[step])
        assert v_dev >= runs.max() - 1e-6, (step, v_dev, runs.max())
        assert polish - v_dev <= 1e-6, (step, polish - v_dev)
        if hybrid:
            assert (picks[step, :dd] == D).all(axis=1).any()
    record_deviation(f"gradient_starts_behind_scipy_dc{dc}_{'hybrid' if hybrid else 'cont'}", behind / total, 1.0)


def test_gradient_refinement_is_deterministic():
    a = _high_dimensional_run(6, True)
    b = _high_dimensional_run(6, True)
    assert np.array_equal(a[1], b[1])
    for ta, tb in zip(a[0]._last_continuous_trace, b[0]._last_continuous_trace):
        assert np.array_equal(ta["starts"], tb["starts"]) and np.array_equal(ta["final"], tb["final"])
        assert np.array_equal(ta["values"], tb["values"], equal_nan=True)
