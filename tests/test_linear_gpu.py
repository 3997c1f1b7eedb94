"""``bbh_linear_moments`` and the Bayesian linear surrogate on the device, against scikit-learn's recorded ``predict(return_std=True)``
and the numpy oracle (tests/_oracle_linear.py), on the fixtures of tests/_linear_cases.py.

Held to:
  moments, every stored case in every form that admits it, and the synthetic edges k = 0 ... 512 against the oracle:
      |mean - ref| <= 4 (k + 4) eps (s (sum_j |coef_j x~_j| + |intercept|) + |ybar|)
      |var  - ref| <= 4 (k + 4) eps s^2 (|x~|^T |Ss| |x~| + 1 / alpha)
    (either side's nested sum errs by at most about (k + 2) eps times the sum of the absolute terms, whatever its order);
  k = 0: the fill values bit for bit; N = 1, 255, 256, 257, a row stride of d + 3 and a duplicated row: equal bits within a form;
  scores of every analytic and MC kind: rtol 1e-9, atol 1e-10 against oracle/gp_oracle.py on the device's own moments (the GP family's bounds);
  end to end: the label the oracle picks from scikit-learn's moments (margins >= 1e-6, checked in tests/test_linear_cpu.py).
Observed maxima are printed and recorded (conftest.record_deviation) in units of their bound."""

import functools

import numpy as np
import pytest

import _linear_cases as lc
import _oracle_linear as ol
from conftest import record_deviation

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-10
AUTO_REGISTER_MAX_KEPT = 16  # form "auto": the register form up to here, the block form above
STORED_FORMS = [(n, f) for n in lc.CASES for f in (("register", "block", "auto") if lc.CASES[n]["kept"] <= 32 else ("block", "auto"))]
SYNTHETIC_FORMS = [(k, f) for k in lc.SYNTHETIC_K for f in (("register", "block") if k <= 32 else ("block",))]


@functools.lru_cache(maxsize=None)
def golden():
    return lc.load_golden()


@functools.lru_cache(maxsize=None)
def synthetic(k):
    return lc.synthetic_model(k)


@functools.lru_cache(maxsize=None)
def engine():
    """One handle for the whole module: ``bbh_linear_moments`` keeps no state, every call brings its tables."""
    from baybe_amd.linear import HipLinearEngine

    return HipLinearEngine(0)


def _packed(g):
    from baybe_amd.linear import check_packed_linear, pack_linear

    packed = pack_linear(lc.as_model(g), g["lo"], g["hi"])
    check_packed_linear(packed, g["X"].shape[1])
    return packed


def _run(g, form, X=None):
    """(mean, var) numpy of the rows ``X`` (a host array or a device tensor; by default the case's candidates) in ``form``."""
    import torch

    eng = engine()
    X = g["X"] if X is None else X
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X)).to(eng._dev())
    mean, var = eng.linear_moments(eng.linear_upload(_packed(g)), X, float(g["ybar"]), float(g["s"]), form)
    return mean.cpu().numpy(), var.cpu().numpy()


def _hold(tag, g, mean, var, ref_mean, ref_var, X=None):
    bm, bv = ol.bounds(g, g["X"] if X is None else X)
    rm, rv = float((np.abs(mean - ref_mean) / bm).max()), float((np.abs(var - ref_var) / bv).max())
    print(tag, "mean", np.abs(mean - ref_mean).max(), f"({rm:.3f} of the bound)", "var", np.abs(var - ref_var).max(), f"({rv:.3f} of the bound)")
    record_deviation(f"linear_moments/{tag}:mean", rm, 1.0)
    record_deviation(f"linear_moments/{tag}:var", rv, 1.0)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert rm <= 1.0 and rv <= 1.0, (tag, rm, rv)


def _expected_form(k, form):
    return "block" if form == "block" or (form == "auto" and k > AUTO_REGISTER_MAX_KEPT) else "register"


# ---- moments ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", STORED_FORMS)
def test_moments_against_scikit_learn(name, form):
    g = golden()[name]
    mean, var = _run(g, form)
    assert engine().linear_last_form() == _expected_form(lc.CASES[name]["kept"], form)
    _hold(f"{name}[{form}]", g, mean, var, *ol.reference_from_sklearn(g))


@pytest.mark.parametrize("k,form", SYNTHETIC_FORMS)
def test_synthetic_edges_against_the_oracle(k, form):
    g = synthetic(k)
    mean, var = _run(g, form)
    assert engine().linear_last_form() == _expected_form(k, form)
    if k == 0:  # the fill: bit for bit
        s, ybar = float(g["s"]), float(g["ybar"])
        assert np.array_equal(mean, np.full(lc.N_CAND, ybar + s * float(g["intercept_"])))
        assert np.array_equal(var, np.full(lc.N_CAND, s * s * (1.0 / float(g["alpha_"]))))
        return
    _hold(f"synthetic_k{k}[{form}]", g, mean, var, *ol.moments(g, g["X"]))


@pytest.mark.parametrize("k,form", [(17, "register"), (17, "block"), (33, "block")])
def test_row_counts_around_a_tile_strides_and_duplicates_give_equal_bits(k, form):
    import torch

    g = synthetic(k)
    X, d = g["X"], g["X"].shape[1]
    mean, var = _run(g, form)
    for N in (1, 255, 256):  # (257 is the full set)
        m, v = _run(g, form, X[:N])
        assert np.array_equal(m, mean[:N]) and np.array_equal(v, var[:N]), N
    # rows read through a stride of d + 3
    wide = torch.full((lc.N_CAND, d + 3), float("nan"), dtype=torch.float64, device=engine()._dev())
    wide[:, :d] = torch.from_numpy(X).to(wide.device)
    view = wide[:, :d]
    assert view.stride(0) == d + 3
    m, v = _run(g, form, view)
    assert np.array_equal(m, mean) and np.array_equal(v, var)
    # a duplicated row: equal bits wherever it sits, and the first index wins
    best = int(np.argmax(mean))
    other = 250 if best != 250 else 100
    X2 = X.copy()
    X2[other] = X2[best]
    dev = torch.from_numpy(X2).to(engine()._dev())
    eng = engine()
    mean2, var2 = eng.linear_moments(eng.linear_upload(_packed(g)), dev, float(g["ybar"]), float(g["s"]), form)
    m2, v2 = mean2.cpu().numpy(), var2.cpu().numpy()
    assert m2[other] == m2[best] == mean[best] and v2[other] == v2[best] == var[best]
    val, idx = eng.argmax(mean2)
    assert idx == min(best, other) and val == mean[best]


def test_bad_arguments_are_refused_with_a_text_and_nothing_runs():
    import torch

    from baybe_amd._lib import HipError

    eng = engine()
    g = synthetic(33)
    X = torch.from_numpy(g["X"]).to(eng._dev())
    tables = eng.linear_upload(_packed(g))
    with pytest.raises(HipError, match="register form holds at most 32"):
        eng.linear_moments(tables, X, 0.0, 1.0, "register")
    bad = dict(tables, cols=tables["cols"].clone())
    bad["cols"][5] = X.shape[1]
    with pytest.raises(HipError, match="outside the d columns"):
        eng.linear_moments(bad, X, 0.0, 1.0, "block")
    with pytest.raises(HipError, match="0 <= k <= 512"):
        eng.linear_moments(dict(tables, k=513), X, 0.0, 1.0, "block")
    m, v = eng.linear_moments(tables, X[:0], 0.0, 1.0, "auto")  # N == 0: a no-op
    assert m.shape == (0,) and v.shape == (0,)
    eng.linear_moments(tables, X, 0.0, 1.0, "auto")
    assert eng.linear_last_form() == "block"
    eng.linear_moments(eng.linear_upload(_packed(synthetic(16))), torch.from_numpy(synthetic(16)["X"]).to(eng._dev()), 0.0, 1.0, "auto")
    assert eng.linear_last_form() == "register"


# ---- scores -----------------------------------------------------------------------------------------------------------------------------
class _Holder:
    """What HipLinearAcq reads of a surrogate."""

    def __init__(self, eng):
        self.engine = eng


@functools.lru_cache(maxsize=None)
def scored():
    """(engine holding the n60_d20 model, resident candidates, the device's own moments as numpy, alive mask) - computed once."""
    import torch

    from baybe_amd.linear import HipLinearEngine

    g = golden()["n60_d20"]
    eng = HipLinearEngine(0)
    eng.set_linear(_packed(g), g["X"].shape[1], float(g["ybar"]), float(g["s"]))
    Xd = torch.from_numpy(g["X"]).to(eng._dev())
    mean, var = eng.posterior(Xd)
    alive = np.ones(lc.N_CAND, dtype=np.uint8)
    alive[[0, 100, 256]] = 0
    return eng, Xd, mean.cpu().numpy(), var.cpu().numpy(), alive


def _close(tag, got, ref, alive=None):
    if alive is not None:
        assert np.array_equal(np.isneginf(got), alive == 0), tag
        got, ref = got[alive == 1], ref[alive == 1]
    dev = float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max())
    print(tag, "max deviation", np.abs(got - ref).max(), f"({dev:.3g} of the allowance)")
    record_deviation(f"linear_scores/{tag}", dev, 1.0)
    assert np.isfinite(got).all() and dev <= 1.0, (tag, dev)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("kind", lc.ANALYTIC_KINDS)
def test_analytic_scores_on_the_devices_own_moments(kind, sign):
    import torch

    from oracle import gp_oracle as go

    eng, Xd, mean, var, alive = scored()
    best = float(np.quantile(sign * mean, 0.7))
    md, vd = eng.posterior(Xd)
    for mask in (None, alive):
        al = None if mask is None else torch.from_numpy(mask).to(Xd.device)
        got = eng.analytic_acq(kind, md, vd, best, sign, 0.4, True, al).cpu().numpy()
        _close(f"{kind}[sign={sign:+.0f},alive={mask is not None}]", got, go.analytic_acq(kind, mean, var, best, sign, 0.4), mask)


@pytest.mark.parametrize("target", ["max", "min", "ramp"])
@pytest.mark.parametrize("kind", lc.MC_KINDS)
def test_mc_scores_on_the_devices_own_moments(kind, target):
    import torch

    import _oracle_objective as oo
    from baybe_amd.linear import HipLinearAcq
    from baybe_amd.objective import ObjectiveProgram
    from oracle import gp_oracle as go

    eng, Xd, mean, var, alive = scored()
    S, seed, beta = 512, 4321, 0.4
    z = go.sobol_normal_base_samples(S, 1, seed)[:, 0]
    if target == "ramp":  # normalized_ramp over the central half of the means, descending
        q25, q75 = np.quantile(mean, [0.25, 0.75])
        ops = (("AFFINE", (-1.0 / (q75 - q25), q75 / (q75 - q25))), ("CLAMP", (0.0, 1.0)))
        sign, prog = 1.0, ObjectiveProgram(ops)
        best = float(np.quantile(oo.apply_program(ops, mean), 0.7))
        ref = oo.q1_scores(kind, ops, mean, var, z, best, beta)
    else:
        sign, prog = (1.0 if target == "max" else -1.0), None
        best = float(np.quantile(sign * mean, 0.7))
        ref = go.mc_acq_q1(kind, mean, var, z, best, sign, beta)
    acq = HipLinearAcq(_Holder(eng), kind, sign, best, S, beta, prog)
    acq.prepare(seed)
    for mask in (None, alive):
        al = None if mask is None else torch.from_numpy(mask).to(Xd.device)
        _close(f"{kind}[{target},alive={mask is not None}]", acq.score(Xd, al).cpu().numpy(), ref, mask)
    from baybe_amd.exceptions import IncompatibleSurrogateError

    with pytest.raises(IncompatibleSurrogateError, match="joint posterior evaluation"):
        acq.prepare(seed, np.zeros((1, 20)))
    with pytest.raises(IncompatibleSurrogateError, match="joint posterior evaluation"):
        acq.greedy(Xd, 2, seed)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _model_arrays(sur, space):
    """The fitted surrogate's scikit-learn model and scaler constants in the layout of a stored case."""
    bounds = space.scaling_bounds.to_numpy(dtype=np.float64)
    m = sur._model
    return dict(lambda_=m.lambda_, threshold_lambda=np.float64(m.threshold_lambda), coef_=m.coef_, intercept_=np.float64(m.intercept_),
                sigma_=m.sigma_, alpha_=np.float64(m.alpha_), lo=bounds[0], hi=bounds[1], ybar=np.float64(sur.engine.ybar),
                s=np.float64(sur.engine.ysd))


@pytest.mark.parametrize("minimize", [False, True])
def test_recommend_end_to_end_returns_the_oracles_labels(minimize, monkeypatch):
    pytest.importorskip("sklearn")
    import copy
    import pickle

    import torch

    from baybe_amd import linear as L
    from baybe_amd.exceptions import IncompatibleSurrogateError
    from baybe_amd.recommenders import HipBotorchRecommender

    space, obj, meas = lc.grid_context(minimize)
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    ref_mean, ref_var, ref_best = lc.grid_oracle_moments(minimize)
    fits = []
    real_fit = L.fit_linear
    monkeypatch.setattr(L, "fit_linear", lambda *a, **k: (fits.append(1), real_fit(*a, **k))[1])
    sur = L.HipBayesianLinearSurrogate()
    for kind in lc.PICK_KINDS:
        want, margin = ol.best_and_margin(lc.grid_oracle_scores(kind, minimize, ref_mean, ref_var, ref_best))
        assert margin >= lc.PICK_MARGIN
        torch.manual_seed(lc.GRID_TORCH_SEED)
        got = HipBotorchRecommender(surrogate_model=sur, acquisition_function=kind).recommend(1, space, obj, meas)
        assert list(got.index) == [want], (kind, minimize)
    assert len(fits) == 1, "a recommend() on unchanged measurements fitted again"
    # the device's moments against scikit-learn's own prediction, and the incumbent
    g = _model_arrays(sur, space)
    mean, var = (t.cpu().numpy() for t in sur.posterior_mean_var(comp))
    _hold(f"grid[minimize={minimize}]", g, mean, var, ref_mean, ref_var, comp)
    sign = -1.0 if minimize else 1.0
    assert abs(sur.engine.best_f(sign) - ref_best) <= ol.bounds(g, sur.engine._X_train)[0].max()
    # read-backs
    some = space.discrete.exp_rep.iloc[::7]
    stats = sur.posterior_stats(some, ("mean", "std", "var", 0.9))
    assert list(stats.columns) == ["y_mean", "y_std", "y_var", "y_Q_0.9"]
    from scipy.stats import norm

    assert np.array_equal(stats["y_mean"].to_numpy(), mean[::7]) and np.array_equal(stats["y_var"].to_numpy(), var[::7])
    assert np.array_equal(stats["y_std"].to_numpy(), np.sqrt(var[::7]))
    assert np.allclose(stats["y_Q_0.9"].to_numpy(), ref_mean[::7] + np.sqrt(ref_var[::7]) * norm.ppf(0.9), rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match="between 0 and 1"):
        sur.posterior_stats(some, (1.5,))
    with pytest.raises(TypeError, match="does not support the statistic"):
        sur.posterior_stats(some, ("mode",))
    best = sur.engine.best_f(sign)
    for kind in lc.PICK_KINDS:
        rec = HipBotorchRecommender(surrogate_model=sur, acquisition_function=kind)
        torch.manual_seed(lc.GRID_TORCH_SEED)
        acq = rec.acquisition_values(some, space, obj, meas)
        _close(f"acquisition_values[{kind},minimize={minimize}]", acq.to_numpy(),
               lc.grid_oracle_scores(kind, minimize, mean[::7], var[::7], best))
        torch.manual_seed(lc.GRID_TORCH_SEED)
        joint = rec.joint_acquisition_value(space.discrete.exp_rep.iloc[[50]], space, obj, meas)
        _close(f"joint_acquisition_value[{kind},minimize={minimize}]", np.array([joint]),
               lc.grid_oracle_scores(kind, minimize, mean[[50]], var[[50]], best))
        with pytest.raises(IncompatibleSurrogateError, match="joint posterior evaluation"):
            rec.joint_acquisition_value(space.discrete.exp_rep.iloc[[5, 50]], space, obj, meas)
    assert len(fits) == 1
    # copies and pickles carry the pack and rebuild their device state on first use
    for twin in (copy.deepcopy(sur), pickle.loads(pickle.dumps(sur))):
        assert twin._engine._handle is None
        m1, v1 = (t.cpu().numpy() for t in twin.posterior_mean_var(comp))
        assert np.array_equal(mean, m1) and np.array_equal(var, v1)
    # non-finite candidates are refused, on the host and on the device, whatever was looked at before
    with pytest.raises(ValueError, match="Non-finite"):
        sur.posterior_mean_var(np.full((1, 3), np.inf))
    Xd = torch.from_numpy(comp).to(sur.engine._dev())
    sur.posterior_mean_var(Xd)
    Xd[7, 1] = float("nan")
    with pytest.raises(ValueError, match="Non-finite"):
        sur.posterior_mean_var(Xd)


def test_transformed_target_rides_on_the_objective_program():
    """An affine (descending) target through the analytic fold and the MC program: the picks of the minimised identity target."""
    pytest.importorskip("sklearn")
    import torch

    from _objective_cases import affine_target
    from _baybe_shim import SingleTargetObjective
    from baybe_amd.linear import HipBayesianLinearSurrogate
    from baybe_amd.recommenders import HipBotorchRecommender

    space, _, meas = lc.grid_context(False)
    obj = SingleTargetObjective(affine_target("y", -1.0, 0.0))
    ref_mean, ref_var, ref_best = lc.grid_oracle_moments(True)  # max of -y: the minimised target
    sur = HipBayesianLinearSurrogate()
    for kind in lc.PICK_KINDS:
        want, _ = ol.best_and_margin(lc.grid_oracle_scores(kind, True, ref_mean, ref_var, ref_best))
        torch.manual_seed(lc.GRID_TORCH_SEED)
        got = HipBotorchRecommender(surrogate_model=sur, acquisition_function=kind).recommend(1, space, obj, meas)
        assert list(got.index) == [want], kind


def test_constant_targets_recommend_the_first_row():
    """No model: every row has the posterior N(ybar + s mean(y~), s^2), every acquisition value ties, the first index wins."""
    from baybe_amd.linear import HipBayesianLinearSurrogate
    from baybe_amd.recommenders import HipBotorchRecommender

    space, obj, meas = lc.grid_context(False)
    meas = meas.copy()
    meas["y"] = 1.25
    sur = HipBayesianLinearSurrogate()
    for kind in lc.PICK_KINDS:
        got = HipBotorchRecommender(surrogate_model=sur, acquisition_function=kind).recommend(1, space, obj, meas)
        assert list(got.index) == [0] and sur._model is None and len(sur.engine.packed["cols"]) == 0
    mean, var = sur.posterior_mean_var(space.discrete.comp_rep.to_numpy(dtype=np.float64)[:5])
    want_mean, want_var = ol.constant_moments(meas["y"].to_numpy())
    assert np.array_equal(mean.cpu().numpy(), np.full(5, want_mean)) and np.array_equal(var.cpu().numpy(), np.full(5, want_var))
    assert (want_mean, want_var) == (1.25, 1.0)
