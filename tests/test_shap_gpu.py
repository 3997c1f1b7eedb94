"""Exact Shapley values on the device against the oracle of tests/_oracle_shap.py (every composed row built explicitly, the oracle
GP's posterior mean as f, the subset formula), per entry, through the C-ABI with fixed hyper-parameters (``bbh_shap_values`` and
``bbh_shap_compose`` / ``bbh_shap_reduce`` / ``bbh_shap_apply`` behind ``HipGP.shap_values``).  Cases and special rows:
tests/_shap_cases.py; their guard and the oracle's: tests/test_shap_cpu.py.

Bound (the issue's, from oracle quantities): ``tol_v = C_BOUND (n + M + 16) eps ysd kmax sum_t |alpha_t|``, ``tol_phi = 2 tol_v``, for
BOTH forms; ``C_BOUND`` from ``profiles/shap_observed_deviations.json`` (tests/_shap_cases.py).  Efficiency - ``sum_g phi + base``
against the mean ``bbh_posterior`` returns for the row, an independent code path - is held to ``(M + 1) tol_phi``.  Where a case has
a column in no feature, that column keeps the background's value in every coalition, the full one included, so the identity's right
side is the mean over b of the posterior mean of (x_r with b's entry in that column)."""

import os

import numpy as np
import pytest

import _oracle_shap as osh
import _shap_cases as sc

pytestmark = pytest.mark.gpu

SWITCHES = ("BBH_SHAP_CPT",)
VARIANTS = {"default": {}, "cpt1": {"BBH_SHAP_CPT": "1"}, "cpt4": {"BBH_SHAP_CPT": "4"}}


@pytest.fixture(scope="module")
def handles():
    from baybe_amd import engine

    keep = {k: os.environ.get(k) for k in SWITCHES}
    made = {}
    try:
        for name, env in VARIANTS.items():
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(env)
            made[name] = engine.HipGP(0)  # (a handle reads the BBH_* switches when it is created)
    finally:
        for k, val in keep.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    yield made
    for g in made.values():
        g.close()


def _load(g, case):
    c = case.build()
    spec, prm = case.device_spec()
    g.set_model(spec, np.array(c.Xt), np.array(c.y))
    g.factorize(prm)
    om = case.oracle_model()
    assert abs(g.ysd - om.ysd) <= 1e-13 * om.ysd and g.jitter == 0.0 and om.jitter == 0.0, (case.id, g.ysd, om.ysd, g.jitter)
    return c


def _record(name, ratio):
    from conftest import record_deviation

    print(f"{name}: observed |device - oracle| / tol(c = 1) = {ratio:.4f} (held to C_BOUND = {sc.C_BOUND})")
    record_deviation(f"shap/{name}", ratio, float(sc.C_BOUND))


def _run(g, case, c, form, X=None):
    phi, base, v = g.shap_values(np.array(c.X) if X is None else X, np.array(c.Bg), case.groups, form=form, want_v=True, n_groups=case.M)
    assert g.shap_last_form() == form
    return phi.cpu().numpy(), base, v.cpu().numpy()


def _ratios(case, phi, base, v):
    ref = case.reference()
    rv = float(np.abs(v - ref.v).max() / ref.tol_v)
    rp = float(np.abs(phi - ref.phi).max() / ref.tol_phi)
    rb = abs(base - ref.base) / ref.tol_v
    return max(rv, rb), rp


def _full_coalition_mean(g, case, c):
    """The mean bbh_posterior returns for x_r - over b with b's entries in the columns of no feature, where the case has such."""
    X, Bg = np.array(c.X), np.array(c.Bg)
    free = case.groups < 0
    if not free.any():
        return g.posterior(X)[0].cpu().numpy()
    rows = np.repeat(X[:, None, :], case.B, axis=1)
    rows[:, :, free] = Bg[None, :, free]
    return g.posterior(rows.reshape(-1, case.d))[0].cpu().numpy().reshape(case.R, case.B).mean(axis=1)


@pytest.mark.parametrize("form", ("fused", "composed"))
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_values_against_oracle(handles, case, form):
    g = handles["default"]
    c = _load(g, case)
    ref = case.reference()
    if form == "composed" and case.M == 5:
        g.SHAP_CHUNK_BYTES = 50_000  # 23 coalitions of 33 rows x 8 columns per posterior pass: uneven chunks of the 544
    try:
        phi, base, v = _run(g, case, c, form)
    finally:
        g.__dict__.pop("SHAP_CHUNK_BYTES", None)
    assert phi.shape == (case.R, case.M) and v.shape == (case.R, 1 << case.M)
    rv, rp = _ratios(case, phi, base, v)
    _record(f"v[{case.id},{form}]", rv)
    _record(f"phi[{case.id},{form}]", rp)
    # efficiency, against the posterior pass
    full = _full_coalition_mean(g, case, c)
    re = float(np.abs(phi.sum(axis=1) + base - full).max() / ((case.M + 1) * ref.tol_phi))
    _record(f"efficiency[{case.id},{form}]", re)
    assert rv <= sc.C_BOUND and rp <= sc.C_BOUND, (case.id, form, rv, rp)
    assert re <= sc.C_BOUND, (case.id, form, re)
    assert base == v[0, 0] and np.all(v[:, 0] == v[0, 0])  # v(r, {}) does not depend on r, bit for bit


def test_reproducibility(handles):
    """Identical explained rows at different positions, two calls, and a row explained alone (R = 1) or inside R = 17: equal bits."""
    case = sc.REPRO_CASE
    g = handles["default"]
    c = _load(g, case)
    phi, base, v = _run(g, case, c, "fused")
    phi2, base2, v2 = _run(g, case, c, "fused")
    assert np.array_equal(phi, phi2) and np.array_equal(v, v2) and base == base2
    assert np.array_equal(phi[3], phi[-1]) and np.array_equal(v[3], v[-1])
    for r in (0, 3, 16):
        pa, ba, va = _run(g, case, c, "fused", X=np.array(c.X[r:r + 1]))
        assert np.array_equal(pa[0], phi[r]) and np.array_equal(va[0], v[r]) and ba == base, r


def test_coalitions_per_thread_instantiations_agree(handles):
    """One and four coalitions per thread (``BBH_SHAP_CPT``; the default picks by size) visit the same sums in the same order."""
    case = sc.CPT_CASE
    out = {}
    for name in ("default", "cpt1", "cpt4"):
        c = _load(handles[name], case)
        out[name] = _run(handles[name], case, c, "fused")
        rv, rp = _ratios(case, *out[name])
        _record(f"v[{case.id},{name}]", rv)
        assert rv <= sc.C_BOUND and rp <= sc.C_BOUND, (name, rv, rp)
    for name in ("cpt1", "cpt4"):
        assert np.array_equal(out[name][0], out["default"][0]) and np.array_equal(out[name][2], out["default"][2]), name


@pytest.mark.parametrize("case,text", [(sc.COMPOSITE_CASE, "needs a single Matern-1/2, Matern-3/2, Matern-5/2 or RBF kernel"),
                                       (sc.ICM_CASE, "needs a single-task model"),
                                       (sc.OVER_N_CASE, r"at most 512 training points \(n = 513\)")], ids=lambda p: getattr(p, "id", ""))
def test_fused_refusals_and_the_composed_answer(handles, case, text):
    from baybe_amd._lib import HipError

    g = handles["default"]
    c = _load(g, case)
    with pytest.raises(HipError, match=text):
        g.shap_values(np.array(c.X), np.array(c.Bg), case.groups, form="fused")
    phi, base, v = g.shap_values(np.array(c.X), np.array(c.Bg), case.groups, form="auto", want_v=True)
    assert g.shap_last_form() == "composed"
    rv, rp = _ratios(case, phi.cpu().numpy(), base, v.cpu().numpy())
    _record(f"v[{case.id},auto]", rv)
    _record(f"phi[{case.id},auto]", rp)
    assert rv <= sc.C_BOUND and rp <= sc.C_BOUND, (case.id, rv, rp)


def test_seventeen_features_are_refused_by_both_forms(handles):
    from baybe_amd._lib import HipError

    case = sc.Case("m17", "matern52", 17, 1, 1, 2, tuple(range(17)))
    g = handles["default"]
    c = _load(g, case)
    for form in ("fused", "auto", "composed"):
        with pytest.raises(HipError, match=r"1 <= M <= 16 features .*M = 17"):
            g.shap_values(np.array(c.X), np.array(c.Bg), case.groups, form=form)
    with pytest.raises(HipError, match="group index of column 2 outside"):
        g.shap_values(np.array(c.X), np.array(c.Bg), case.groups, form="fused", n_groups=2)


# ---- through the public surface -----------------------------------------------------------------------------------------------------
def test_insight_on_a_gp_surrogate():
    from baybe_amd.insights import HipSHAPInsight, shapley_values
    from baybe_amd.surrogates import HipGaussianProcessSurrogate

    space, meas, objective = sc.surface_problem()
    sur = HipGaussianProcessSurrogate()
    sur.fit(space, objective, meas)
    bg = meas[["x", "c"]]
    data = meas[["c", "t", "x"]].iloc[:5]
    ins = HipSHAPInsight.from_surrogate(sur, bg)
    (ex,) = ins.explain(data)
    assert ex.feature_names == ["c", "x"] and ex.values.shape == (5, 2)  # M = 2 in the experimental representation
    phi, base, names = shapley_values(sur, data, bg)
    assert names == ["x", "c"] and np.array_equal(ex.values, phi[:, [1, 0]]) and np.all(ex.base_values == base)
    assert sur.engine.shap_last_form() == "fused"
    # ... against the oracle under the device's fitted hyper-parameters
    from oracle import gp_oracle as go

    prm = sur.engine.params
    comp = space.transform(meas).to_numpy(float)
    om = go.fit_gp(go.GPSpec.baybe_default(4, np.zeros(4), np.ones(4)), comp, meas["t"].to_numpy(),
                   go.GPParams(prm.lengthscale, prm.noise, prm.mean))
    ref = osh.explain(om, comp[:5], comp, np.array([0, 1, 1, 1]), 2)
    cond = np.linalg.cond(om.L @ om.L.T)  # (a fitted model, not a hand-set one: the error of the solve for alpha is cond eps |alpha|, i.e. cond / (n + M + 16) = cond / 30 in units of tol at c = 1)
    assert np.abs(phi - ref.phi).max() <= max(sc.C_BOUND, cond / 30.0) * ref.tol_phi
    mean = sur.posterior_stats(data, stats=("mean",))["t_mean"].to_numpy()
    assert np.abs(phi.sum(axis=1) + base - mean).max() <= 3 * max(sc.C_BOUND, cond / 30.0) * ref.tol_phi
    # M = 4 in the computational representation, in the caller's column order
    comp_bg = space.transform(bg)
    ins4 = HipSHAPInsight.from_surrogate(sur, comp_bg, "ExactExplainer", use_comp_rep=True)
    order = ["c_b", "x", "c_c", "c_a"]
    (ex4,) = ins4.explain(comp_bg[order].iloc[:5])
    phi4, base4, names4 = shapley_values(sur, comp_bg.iloc[:5], comp_bg, use_comp_rep=True)
    assert names4 == ["x", "c_a", "c_b", "c_c"] and ex4.feature_names == order and ex4.values.shape == (5, 4)
    assert np.array_equal(ex4.values, phi4[:, [names4.index(n) for n in order]])
    assert abs(base4 - base) <= ref.tol_v * max(sc.C_BOUND, cond / 30.0)
    # the composed form answers the same question
    phi_c, base_c, _ = shapley_values(sur, data, bg, form="composed")
    assert sur.engine.shap_last_form() == "composed"
    assert np.abs(phi_c - phi).max() <= 2 * sc.C_BOUND * ref.tol_phi and abs(base_c - base) <= 2 * sc.C_BOUND * ref.tol_v


def test_insight_on_a_replicated_surrogate():
    from baybe_amd.insights import HipSHAPInsight, shapley_values
    from baybe_amd.surrogates import HipGaussianProcessSurrogate

    space, meas, objective = sc.surface_problem(two_targets=True)
    comp = HipGaussianProcessSurrogate().replicate()
    comp.fit(space, objective, meas)
    ins = HipSHAPInsight.from_surrogate(comp, meas[["x", "c"]])
    out = ins.explain(meas[["x", "c"]].iloc[:3])
    assert isinstance(out, tuple) and len(out) == 2 and all(e.values.shape == (3, 2) for e in out)
    for k, e in enumerate(out):
        phi, base, _ = shapley_values(comp.models[k], meas.iloc[:3], meas)
        assert np.array_equal(e.values, phi) and np.all(e.base_values == base)
    assert not np.array_equal(out[0].values, out[1].values)


def test_insight_on_a_forest_surrogate():
    """The composed form over the forest's own posterior: held to the oracle formula applied to the device's ``forest_predict`` means
    of the composed rows - summation error only."""
    from baybe_amd.forest import HipRandomForestSurrogate
    from baybe_amd.insights import HipSHAPInsight
    from baybe_amd._lib import HipError

    space, meas, objective = sc.surface_problem()
    sur = HipRandomForestSurrogate(model_params={"n_estimators": 20, "random_state": 0})
    sur.fit(space, objective, meas)
    bg = meas[["x", "c"]]
    (ex,) = HipSHAPInsight.from_surrogate(sur, bg).explain(bg.iloc[:4])
    eng = sur.engine
    assert eng.shap_last_form() == "composed"
    comp = space.transform(meas).to_numpy(float)
    f = lambda rows: eng.predict(np.ascontiguousarray(rows)).cpu().numpy().mean(axis=0)  # noqa: E731
    v = osh.coalition_values(f, comp[:4], comp, np.array([0, 1, 1, 1]), 2)
    phi = osh.subset_shapley(v, 2)
    scale = np.abs(f(comp)).max()
    assert np.abs(ex.values - phi).max() <= 1e-12 * scale and np.abs(ex.base_values - v[0, 0]).max() <= 1e-12 * scale
    assert np.abs(ex.values).max() > 1e-3 * scale  # (the explanation is not trivially zero)
    with pytest.raises(HipError, match="the fused form needs a Gaussian process model"):
        HipSHAPInsight.from_surrogate(sur, bg, form="fused").explain(bg.iloc[:1])
