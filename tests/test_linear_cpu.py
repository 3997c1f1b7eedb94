"""Host side of the Bayesian linear (ARD) surrogate, and the fixtures the GPU tests stand on: the numpy oracle equals scikit-learn's own
``predict(return_std=True)`` within the summation bound, the committed golden file equals a fresh fit, the packed triangular form equals
the full quadratic form, malformed packs are refused, pack / engine / surrogate survive a copy and a pickle, ``model_params`` follows
the reference's table, constant targets are judged on the standardised targets, every refusal happens before a fit, and every pick of
the end-to-end GPU tests is decided by a margin of 1e-6."""

import copy
import functools
import pickle

import numpy as np
import pytest

import _linear_cases as lc
import _oracle_linear as ol
from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, ParetoObjective, SearchSpace, SingleTargetObjective, TaskParameter
from baybe_amd import linear as L
from baybe_amd.exceptions import IncompatibilityError, IncompatibleAcquisitionFunctionError, IncompatibleSurrogateError


@functools.lru_cache(maxsize=None)
def golden():
    return lc.load_golden()


# ---- oracle and golden file -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CASES))
def test_oracle_equals_scikit_learn_within_the_summation_bound(name):
    g = golden()[name]
    c = lc.CASES[name]
    keep = g["lambda_"] < g["threshold_lambda"]
    assert int(keep.sum()) == c["kept"] and g["X"].shape == (lc.N_CAND, c["d"]) and g["sigma_"].shape == (c["kept"], c["kept"])
    assert (c["n"] < c["d"]) == c["woodbury"] and np.array_equal(g["coef_"][~keep], np.zeros(int((~keep).sum())))
    mean, var = ol.moments(g, g["X"])
    ref_mean, ref_var = ol.reference_from_sklearn(g)
    bm, bv = ol.bounds(g, g["X"])
    print(name, "mean", np.abs(mean - ref_mean).max(), "of", bm.min(), "var", np.abs(var - ref_var).max(), "of", bv.min())
    assert (np.abs(mean - ref_mean) <= bm).all() and (np.abs(var - ref_var) <= bv).all()
    assert (var > 0).all()


def test_woodbury_sigma_is_not_exactly_symmetric():
    """What the symmetrisation in the pack is for."""
    asym = {n: np.abs(golden()[n]["sigma_"] - golden()[n]["sigma_"].T).max() for n in lc.CASES if lc.CASES[n]["woodbury"]}
    assert all(0.0 < a < 1e-10 for a in asym.values()), asym


def test_golden_file_equals_a_fresh_fit():
    pytest.importorskip("sklearn")
    import importlib.util

    assert lc.GOLDEN.stat().st_size < 1024 * 1024
    spec = importlib.util.spec_from_file_location("make_linear_golden", lc.GOLDEN.parent / "make_linear_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.build()
    with np.load(lc.GOLDEN) as z:
        assert sorted(z.files) == sorted(fresh)
        for key in z.files:
            assert np.array_equal(z[key], fresh[key]), key


# ---- pack -------------------------------------------------------------------------------------------------------------------------------
def _models():
    for name in lc.CASES:
        yield name, golden()[name]
    for k in lc.SYNTHETIC_K:
        yield f"synthetic_k{k}", lc.synthetic_model(k)


@pytest.mark.parametrize("name,g", list(_models()), ids=[n for n, _ in _models()])
def test_packed_triangular_form_equals_the_quadratic_form(name, g):
    packed = L.pack_linear(lc.as_model(g), g["lo"], g["hi"])
    d = g["X"].shape[1]
    L.check_packed_linear(packed, d)
    keep = g["lambda_"] < g["threshold_lambda"]
    k = int(keep.sum())
    assert np.array_equal(packed["cols"], np.nonzero(keep)[0]) and packed["cols"].dtype == np.int32 and packed["T"].shape == (k, k)
    assert np.array_equal(packed["coef"], g["coef_"][keep]) and np.array_equal(packed["range"], (g["hi"] - g["lo"])[keep])
    assert packed["intercept"] == float(g["intercept_"]) and packed["inv_alpha"] == 1.0 / float(g["alpha_"])
    assert not np.triu(packed["T"], 1).any()
    xs = (g["X"][:, packed["cols"]] - packed["lo"]) / packed["range"]
    quad_T = np.einsum("ni,ij,nj->n", xs, packed["T"], xs)
    quad_S = np.einsum("ni,ij,nj->n", xs, g["sigma_"].reshape(k, k), xs)
    Ss = np.abs((g["sigma_"].reshape(k, k) + g["sigma_"].reshape(k, k).T) / 2.0)
    bound = 4 * (k + 4) * ol.EPS * np.einsum("ni,ij,nj->n", np.abs(xs), Ss, np.abs(xs))
    assert (np.abs(quad_T - quad_S) <= bound).all()
    # ... and the pack reproduces the oracle's moments
    mean, var = ol.moments(g, g["X"])
    s, ybar = float(g["s"]), float(g["ybar"])
    bm, bv = ol.bounds(g, g["X"])
    assert (np.abs(ybar + s * (xs @ packed["coef"] + packed["intercept"]) - mean) <= bm).all()
    assert (np.abs(s * s * (quad_T + packed["inv_alpha"]) - var) <= bv).all()


def test_constant_pack():
    packed = L.constant_linear(0.25)
    L.check_packed_linear(packed, 0)
    L.check_packed_linear(packed, 5)
    assert len(packed["cols"]) == 0 and packed["T"].shape == (0, 0) and (packed["intercept"], packed["inv_alpha"]) == (0.25, 1.0)


def test_check_packed_linear_refuses_what_the_kernel_would_misread():
    g = golden()["n40_d6"]
    good = L.pack_linear(lc.as_model(g), g["lo"], g["hi"])
    L.check_packed_linear(good, 6)

    def bad(**changes):
        out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        out.update(changes)
        return out

    T_upper = good["T"].copy()
    T_upper[0, 1] = 1e-3
    rng0 = good["range"].copy()
    rng0[2] = 0.0
    coef_nan = good["coef"].copy()
    coef_nan[1] = np.nan
    cols_out = good["cols"].copy()
    cols_out[-1] = 6
    for pack, d, match in ((bad(T=T_upper), 6, "lower triangular"), (bad(range=rng0), 6, "not positive"), (bad(coef=coef_nan), 6, "not finite"),
                           (bad(inv_alpha=np.inf), 6, "not finite"), (bad(cols=cols_out), 6, "outside"), (good, 5, "outside"),
                           (bad(cols=good["cols"].astype(np.int64)), 6, "int32"), (bad(lo=good["lo"][:-1]), 6, "one entry"),
                           (bad(T=good["T"][:-1]), 6, r"\[k, k\]")):
        with pytest.raises(ValueError, match=match):
            L.check_packed_linear(pack, d)
    big = lc.synthetic_model(513)
    with pytest.raises(ValueError, match="at most 512"):
        L.check_packed_linear(L.pack_linear(lc.as_model(big), big["lo"], big["hi"]), 521)


def _engine_without_device(packed, d):
    eng = L.HipLinearEngine.__new__(L.HipLinearEngine)
    eng.__setstate__({"device": 0, "spec": None, "params": None, "n": 0, "ybar": -1.5, "ysd": 2.5, "jitter": 0.0, "X_train": np.zeros((2, d)),
                      "y_train": np.zeros(2), "model_args": None, "linear": (packed, d, "auto")})
    return eng


def _same_pack(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_pack_engine_and_surrogate_survive_a_copy_and_a_pickle():
    g = golden()["n60_d20"]
    packed = L.pack_linear(lc.as_model(g), g["lo"], g["hi"])
    for twin in (copy.deepcopy(packed), pickle.loads(pickle.dumps(packed))):
        assert _same_pack(packed, twin)
    eng = _engine_without_device(packed, 20)
    for twin in (copy.deepcopy(eng), pickle.loads(pickle.dumps(eng))):
        assert _same_pack(twin.packed, packed) and (twin.d, twin.ybar, twin.ysd, twin.form) == (20, -1.5, 2.5, "auto")
        assert twin._handle is None and twin._L is None and twin._copied and not twin._restorable
        assert np.array_equal(twin._X_train, np.zeros((2, 20)))
    sur = L.HipBayesianLinearSurrogate(model_params={"max_iter": 50})
    sur._engine, sur._measurements_hash = eng, ("key",)
    for twin in (copy.deepcopy(sur), pickle.loads(pickle.dumps(sur))):
        assert twin.model_params == {"max_iter": 50} and twin._measurements_hash == ("key",) and _same_pack(twin._engine.packed, packed)


# ---- the surrogate's host side -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [{"max_iter": 5}, {"tol": 1e-4}, {"alpha_1": 1e-5, "alpha_2": 1e-5, "lambda_1": 1e-5, "lambda_2": 1e-5},
                                    {"compute_score": True}, {"threshold_lambda": 1e3}, {"fit_intercept": False}, {"copy_X": True},
                                    {"verbose": False}])
def test_valid_model_params(params):
    assert L.HipBayesianLinearSurrogate(model_params=params).model_params == params


@pytest.mark.parametrize("params", [{"max_iter": 5.3}, {"max_iter": True}, {"tol": 1}, {"tol": "1e-3"}, {"compute_score": 1}, {"fit_intercept": None},
                                    {"bla": None}, {"n_estimators": 5}, {"threshold_lambda": None}, {"verbose": 2}])
def test_invalid_model_params(params):
    with pytest.raises(TypeError, match="The provided dictionary for 'model_params' is invalid."):
        L.HipBayesianLinearSurrogate(model_params=params)


def test_class_surface_and_plugin_layout():
    import _baybe_layout as bl
    import baybe_amd
    from baybe_amd import plugin
    from baybe_amd.exceptions import ModelNotTrainedError

    S = L.HipBayesianLinearSurrogate
    assert baybe_amd.HipBayesianLinearSurrogate is S and baybe_amd.make_baybe_linear_surrogate is plugin.make_baybe_linear_surrogate
    assert {"HipBayesianLinearSurrogate", "make_baybe_linear_surrogate"} <= set(baybe_amd.__all__)
    s = S()
    assert s.model_params == {} and s.device == 0 and not hasattr(s, "__dict__")
    assert (S.supports_transfer_learning, S.supports_multi_output, S.is_independent_gaussian) == (False, False, True)
    assert not getattr(S, "is_ensemble", False)
    with pytest.raises(IncompatibilityError, match="BoTorch"):
        s.to_botorch()
    with pytest.raises(IncompatibilityError, match="BoTorch posterior"):
        s._posterior(None)
    with pytest.raises(NotImplementedError):
        s._fit(None, None)
    with pytest.raises(ModelNotTrainedError):
        s.posterior_mean_var(np.zeros((1, 1)))
    B = plugin.make_baybe_linear_surrogate(bl.Surrogate)
    b = B(model_params={"max_iter": 3})
    assert isinstance(b, bl.Surrogate) and issubclass(B, bl.Surrogate) and issubclass(B, L.HipLinearSurrogateImpl) and not hasattr(b, "__dict__")
    assert b._searchspace is None and b._measurements_hash is None and B.is_independent_gaussian and B.fit is L.HipLinearSurrogateImpl.fit
    with pytest.raises(TypeError, match="invalid"):
        B(model_params={"max_iter": 5.3})


def test_constant_targets_are_judged_on_the_standardised_targets():
    """``catch_constant_targets`` wraps ``_fit``: n = 1, an exactly constant y and a y with deviation 1e-9 fit no model; the posterior
    is ``ybar + s mean(y~)`` with variance ``s^2`` (s = 1 in all three).  A y with deviation 1e-7 is standardised to deviation 1 and IS
    fitted, though its raw deviation is below 1e-6."""
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(3)
    x = rng.random((6, 2))
    lo, hi = np.zeros(2), np.ones(2)
    tiny = 2.0 + 1e-9 * np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0]) / np.sqrt(1.2)
    assert abs(np.std(tiny, ddof=1) - 1e-9) < 1e-12
    for y in (np.array([3.5]), np.full(6, 2.0), tiny):
        packed, ybar, s, model = L.fit_linear(x[: len(y)], y, lo, hi, {})
        assert model is None and len(packed["cols"]) == 0 and packed["inv_alpha"] == 1.0 and s == 1.0
        L.check_packed_linear(packed, 2)
        want_mean, want_var = ol.constant_moments(y)
        assert ybar + s * packed["intercept"] == want_mean and s * s * packed["inv_alpha"] == want_var == 1.0
        assert abs(want_mean - y.mean()) <= 1e-15
    y = 2.0 + 1e-7 * rng.standard_normal(6)
    packed, ybar, s, model = L.fit_linear(x, y, lo, hi, {})
    assert model is not None and s < 1e-6 and packed["inv_alpha"] != 1.0
    y_std, _, _ = L.standardize_targets(y)
    assert not L.is_constant_target(y_std) and L.is_constant_target(np.array([0.0, 1e-6])) and not L.is_constant_target(np.array([0.0, 1e-5]))
    with pytest.raises(ValueError, match="no extent"):
        L.fit_linear(x, rng.random(6), lo, np.array([1.0, 0.0]), {})


def _context():
    vals = np.arange(6) / 5.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(2)])
    meas = space.discrete.exp_rep.iloc[[1, 7, 20, 33]].copy()
    meas["y"] = [0.1, 0.4, 0.3, 0.2]
    return space, SingleTargetObjective(NumericalTarget("y")), meas


def test_every_refusal_happens_before_a_fit(monkeypatch):
    from baybe_amd.recommenders import HipBotorchRecommender

    def no_fit(self, *a, **k):
        raise AssertionError("fit() was called")

    monkeypatch.setattr(L.HipLinearSurrogateImpl, "fit", no_fit)
    space, obj, meas = _context()

    def rec(**kw):
        return HipBotorchRecommender(surrogate_model=L.HipBayesianLinearSurrogate(), **kw)

    # task parameters: the base class's ValueError
    tasks = SearchSpace.from_product([NumericalDiscreteParameter("x0", np.arange(3) / 2.0), TaskParameter("t", ("a", "b"))])
    tmeas = tasks.discrete.exp_rep.iloc[[0, 3]].copy()
    tmeas["y"] = [0.1, 0.2]
    with pytest.raises(ValueError, match=r"task parameters but the selected surrogate model type \(HipBayesianLinearSurrogate\)"):
        rec().recommend(1, tasks, obj, tmeas)
    # continuous / hybrid spaces
    hybrid = SearchSpace(space.discrete)
    hybrid.continuous = type("Cont", (), {"is_empty": False})()
    for call in (lambda r: r.recommend(1, hybrid, obj, meas), lambda r: r.acquisition_values(meas, hybrid, obj, meas)):
        with pytest.raises(NotImplementedError, match="non-GP"):
            call(rec())
    # multi-target objectives
    pareto = ParetoObjective([NumericalTarget("y"), NumericalTarget("z")])
    with pytest.raises(IncompatibleSurrogateError, match="single-output"):
        rec()._setup_botorch_acqf(space, pareto, meas)
    # multi-output acquisition functions and the noisy forms
    for name in ("qNEI", "qLogNEI", "qLogNEHVI", "qNEHVI", "qLogNParEGO"):
        with pytest.raises(IncompatibleAcquisitionFunctionError):
            rec(acquisition_function=name)._setup_botorch_acqf(space, obj, meas)
    # batches and pending experiments: no joint posterior
    pending = space.discrete.exp_rep.iloc[[2]]
    for call in (lambda r: r.recommend(2, space, obj, meas), lambda r: r.recommend(1, space, obj, meas, pending_experiments=pending),
                 lambda r: r._setup_botorch_acqf(space, obj, meas, pending),
                 lambda r: r.acquisition_values(meas, space, obj, meas, pending_experiments=pending)):
        for kw in ({}, {"acquisition_function": "EI"}, {"acquisition_function": "qUCB"}):
            with pytest.raises(IncompatibleSurrogateError, match="joint posterior evaluation"):
                call(rec(**kw))
    # row shards
    with pytest.raises(IncompatibilityError, match="[Rr]ow shards"):
        rec(shard=object())._setup_botorch_acqf(space, obj, meas)
    # (and what is not refused does reach the fit - a transformed single target included)
    from _objective_cases import affine_target, bell_target

    for objective, kw in ((obj, {}), (obj, {"acquisition_function": "UCB"}), (SingleTargetObjective(bell_target("y", 0.3, 0.2)), {}),
                          (SingleTargetObjective(affine_target("y", -2.0, 1.0)), {"acquisition_function": "EI"})):
        with pytest.raises(AssertionError, match="fit"):
            rec(**kw).recommend(1, space, objective, meas)
    # a non-affine transformation under an analytic acquisition function: the existing refusal, also before a fit
    with pytest.raises(IncompatibilityError, match="non-Gaussian"):
        rec(acquisition_function="EI").recommend(1, space, SingleTargetObjective(bell_target("y", 0.3, 0.2)), meas)


def test_surrogate_fit_refusals_use_the_references_texts():
    s = L.HipBayesianLinearSurrogate()
    space, obj, meas = _context()
    with pytest.raises(IncompatibleSurrogateError, match="single-output surrogate in a 2-target multi-output context"):
        s.fit(space, ParetoObjective([NumericalTarget("y"), NumericalTarget("z")]), meas)
    tasks = type("Tasks", (), {"n_tasks": 2, "task_idx": 0, "comp_rep_columns": space.comp_rep_columns, "scaling_bounds": space.scaling_bounds})()
    with pytest.raises(ValueError, match=r"task parameters but the selected surrogate model type \(HipBayesianLinearSurrogate\)"):
        s.fit(tasks, obj, meas)
    bad = meas.copy()
    bad.loc[bad.index[0], "x0"] = np.inf
    with pytest.raises(ValueError, match="Non-finite values among the training rows"):
        s.fit(space, obj, bad)
    bad = meas.copy()
    bad.loc[bad.index[0], "y"] = np.nan
    with pytest.raises(ValueError, match="Missing target values"):
        s.fit(space, obj, bad)


# ---- the condition on the end-to-end fixture -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minimize", [False, True])
@pytest.mark.parametrize("kind", lc.PICK_KINDS)
def test_every_end_to_end_pick_clears_the_margin(kind, minimize):
    """Best minus second-best oracle score >= 1e-6 for every pick the GPU test compares: the device's 1e-9 deviations cannot change one."""
    pytest.importorskip("sklearn")
    scores = lc.grid_oracle_scores(kind, minimize)
    pick, margin = ol.best_and_margin(scores)
    print(kind, minimize, pick, margin)
    assert np.isfinite(scores).all() and margin >= lc.PICK_MARGIN, (kind, minimize, margin)
