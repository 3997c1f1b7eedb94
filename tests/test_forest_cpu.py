"""Host side of the random forest surrogate, and the fixtures the GPU tests stand on: the numpy oracle equals scikit-learn bit for bit,
the packed layout round-trips, the committed golden file equals a fresh fit, the count-weighted score equals the per-sample one, the
member draw is reproducible and private, ``model_params`` follows the reference's table, constant targets fall back to one leaf, every
refusal happens before a fit, and every greedy step of every fixture is decided by a margin the device cannot blur.  The forest of
production-sized trees (``MIXED``) has its own file: it equals a fresh fit, has the node counts it is for, and its 63-point pending
blocks leave the candidate its say."""

import functools
import math

import numpy as np
import pytest

import _forest_cases as fc
import _oracle_forest as of
from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, ParetoObjective, SearchSpace, SingleTargetObjective
from baybe_amd import forest as F
from baybe_amd.exceptions import IncompatibilityError, IncompatibleAcquisitionFunctionError, IncompatibleSurrogateError

MARGIN = 1e-8


@functools.lru_cache(maxsize=None)
def golden():
    return fc.load_golden()


@functools.lru_cache(maxsize=None)
def oracle_predictions(name):
    g = golden()[fc.stored_name(name)]
    return of.traverse(g["packed"], g["X"]), of.traverse(g["packed"], g["train_x"])


# ---- traversal and layout --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in fc.CASES if "like" not in fc.CASES[n]])
def test_oracle_traversal_equals_scikit_learn_bit_for_bit(name):
    """Against the recorded ``estimator.predict`` outputs and, where scikit-learn is importable, a fresh ``predict`` - threshold rows
    (float32 cast on the other side of the float64 value) included."""
    g = golden()[name]
    P, Ptrain = oracle_predictions(name)
    assert np.array_equal(P, g["pred"]) and np.array_equal(Ptrain, g["pred_train"])
    pytest.importorskip("sklearn")
    estimators, X, train_x, _ = fc.fit_case(name)
    assert np.array_equal(of.traverse(F.pack_forest(estimators), X), np.stack([e.predict(X) for e in estimators]))


def test_threshold_rows_take_the_other_side_in_float64():
    """The fixture does what it is for: comparing the float64 value instead of its float32 cast changes predictions."""
    g = golden()["threshold"]
    X, packed = g["X"], g["packed"]
    assert (X.astype(np.float32).astype(np.float64) != X).any()
    wrong = dict(packed)
    P64 = _traverse_float64(wrong, X)
    assert (P64 != g["pred"]).any()


def _traverse_float64(packed, X):
    off = packed["offsets"]
    P = np.empty((len(off) - 1, len(X)))
    for t in range(len(off) - 1):
        sl = slice(off[t], off[t + 1])
        left, right, feat, thr, val = (packed[k][sl] for k in ("children_left", "children_right", "feature", "threshold", "value"))
        for i, x in enumerate(X):
            node = 0
            while left[node] >= 0:
                node = left[node] if x[feat[node]] <= thr[node] else right[node]
            P[t, i] = val[node]
    return P


def test_pack_forest_round_trips_and_assumes_no_child_position():
    pytest.importorskip("sklearn")
    estimators, X, _, _ = fc.fit_case("bestfirst")
    packed = F.pack_forest(estimators)
    trees = F.unpack_forest(packed)
    assert len(trees) == len(estimators) and packed["offsets"][-1] == sum(e.tree_.node_count for e in estimators)
    for tree, est in zip(trees, estimators):
        t = est.tree_
        assert np.array_equal(tree["children_left"], t.children_left) and np.array_equal(tree["children_right"], t.children_right)
        assert np.array_equal(tree["feature"], t.feature) and np.array_equal(tree["threshold"], t.threshold)
        assert np.array_equal(tree["value"], t.value[:, 0, 0])
    inner = packed["children_left"] >= 0
    first = np.repeat(packed["offsets"][:-1], np.diff(packed["offsets"]))
    local = np.arange(len(inner)) - first
    assert (packed["children_left"][inner] != local[inner] + 1).any(), "a best-first forest whose left child is always node + 1"
    F.check_packed(packed, X.shape[1])
    # stumps plus a single-leaf tree
    stumps = golden()["stumps"]["packed"]
    sizes = np.diff(stumps["offsets"])
    assert list(sizes) == [3, 3, 1] and stumps["children_left"][-1] == -1


def test_check_packed_refuses_what_the_kernels_would_misread():
    good = golden()["n65_d3_t7"]["packed"]
    F.check_packed(good, 3)
    inner = np.nonzero(good["children_left"] >= 0)[0]
    for key, value, match in (("feature", 3, "feature"), ("children_left", 10_000, "outside its tree"), ("children_right", -1, "one child")):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][inner[0]] = value
        with pytest.raises(ValueError, match=match):
            F.check_packed(bad, 3)
    with pytest.raises(ValueError, match="feature"):
        F.check_packed(good, 2)


def test_golden_file_equals_a_fresh_fit():
    pytest.importorskip("sklearn")
    import importlib.util

    assert fc.GOLDEN.stat().st_size < 100 * 1024
    spec = importlib.util.spec_from_file_location("make_forest_golden", fc.GOLDEN.parent / "make_forest_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.build()
    with np.load(fc.GOLDEN) as z:
        assert sorted(z.files) == sorted(fresh)
        for key in z.files:
            assert np.array_equal(z[key], fresh[key]), key


@functools.lru_cache(maxsize=None)
def mixed():
    return fc.load_mixed()


def test_mixed_file_equals_a_fresh_fit():
    pytest.importorskip("sklearn")
    import importlib.util

    assert fc.MIXED_GOLDEN.stat().st_size < 100 * 1024
    spec = importlib.util.spec_from_file_location("make_forest_golden", fc.GOLDEN.parent / "make_forest_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.build_mixed()
    with np.load(fc.MIXED_GOLDEN) as z:
        assert sorted(z.files) == sorted(fresh)
        for key in z.files:
            assert np.array_equal(z[key], fresh[key]), key


def test_mixed_forest_has_the_sizes_it_is_for_and_the_oracle_walks_it_as_scikit_learn_did():
    """One tree ending in each 256-node staging slot, one at the 1023-node edge, two above the budget in the 2nd and 4th position, a
    single leaf last; thresholds exact in float32; ``check_packed`` accepts it; the oracle's walk equals the recorded ``predict``."""
    from baybe_amd import _lib

    g = mixed()
    packed = g["packed"]
    budget = int(_lib.load_library().bbh_forest_lds_nodes())
    sizes = tuple(int(n) for n in np.diff(packed["offsets"]))
    assert sizes == fc.MIXED_NODES == (199, 1025, 399, 1399, 659, 1023, 899, 1) and budget == 1024
    assert sorted({(n - 1) // 256 for n in sizes if 1 < n <= budget}) == [0, 1, 2, 3]
    assert g["X"].shape == (257, 4) and g["train_x"].shape == (700, 4) and len(np.unique(g["train_x"], axis=0)) == 700
    assert g["pred"].shape == (8, 257) and g["pred_train"].shape == (8, 700)
    inner = packed["children_left"] >= 0
    assert np.array_equal(packed["threshold"][inner].astype(np.float32).astype(np.float64), packed["threshold"][inner])
    F.check_packed(packed, 4)
    assert np.array_equal(of.traverse(packed, g["X"]), g["pred"]) and np.array_equal(of.traverse(packed, g["train_x"]), g["pred_train"])
    assert sorted(g) == ["X", "packed", "pred", "pred_train", "train_x"]


def test_over_budget_tree_exceeds_the_exported_budget():
    """The fixture of the global-memory path really has more nodes per tree than the kernels stage into LDS."""
    pytest.importorskip("sklearn")
    from baybe_amd import _lib

    budget = int(_lib.load_library().bbh_forest_lds_nodes())
    estimators, _, _, _ = fc.fit_case("big", fc.BIG)
    assert budget == 1024 and min(e.tree_.node_count for e in estimators) > budget


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_count_weighted_score_equals_the_per_sample_score(name):
    c = fc.case(name)
    P, Ptrain = oracle_predictions(name)
    idx = F.ensemble_member_indices(c["S"], P.shape[0], c["sampler"])
    counts = F.ensemble_member_counts(c["S"], P.shape[0], c["sampler"])
    assert np.array_equal(counts, np.bincount(idx, minlength=P.shape[0])) and counts.sum() == c["S"] and counts.dtype == np.int32
    if c["S"] < P.shape[0]:
        assert (counts == 0).any()
    best = of.best_f(Ptrain, c["sign"])
    # rtol 1e-12, plus the absolute error two fp64 sums of S terms may differ by where a score is a difference of such sums (qSR of
    # mixed signs, |obj - m| of qUCB / qPSTD for a row the trees agree on): 4 S 2^-53 max(1, |obj|, |best_f|)
    atol = 4 * c["S"] * 2.0**-53 * max(1.0, np.abs(P).max(), abs(best))
    for k in fc.PENDING:
        pend = P[:, fc.pending_rows(c["N"], k)] if k else None
        for kind in fc.MC_KINDS:
            a = of.scores(kind, P, pend, idx, best, c["sign"])
            b = of.scores_from_counts(kind, P, pend, counts, best, c["sign"])
            assert np.allclose(a, b, rtol=1e-12, atol=atol), (name, kind, k, np.abs(a - b).max())


def test_ensemble_member_indices_is_reproducible_in_range_and_private():
    import torch

    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    a = F.ensemble_member_indices(512, 7, 99)
    assert torch.equal(torch.get_rng_state(), before), "the global generator moved"
    b = F.ensemble_member_indices(512, 7, 99)
    assert np.array_equal(a, b) and a.shape == (512,) and a.min() >= 0 and a.max() < 7 and a.dtype == np.int64
    assert not np.array_equal(a, F.ensemble_member_indices(512, 7, 100))
    with torch.random.fork_rng(devices=[]):  # the documented form of the draw
        torch.manual_seed(99)
        assert np.array_equal(a, torch.randint(0, 7, (512,)).numpy())
    assert set(F.ensemble_member_indices(5, 1, 3)) == {0}


# ---- the surrogate's host side ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [{"n_estimators": 5}, {"criterion": "squared_error"}, {"max_features": 0.4}, {"monotonic_cst": None}])
def test_valid_model_params(params):
    """The forest rows of the reference's table of valid ``model_params`` (tests/test_surrogate.py:113-116)."""
    assert F.HipRandomForestSurrogate(model_params=params).model_params == params


@pytest.mark.parametrize("params", [{"n_estimators": 5.3}, {"criterion": "squared_error123"}, {"max_features": True},
                                    {"min_samples_split": None}, {"bla": None}, {"n_estimators": True}, {"ccp_alpha": 1},
                                    {"bootstrap": 1}])
def test_invalid_model_params(params):
    """The forest rows of the reference's table of invalid ``model_params`` (tests/test_surrogate.py:134-144), plus int-for-float,
    bool-for-int and int-for-bool."""
    with pytest.raises(TypeError, match="The provided dictionary for 'model_params' is invalid."):
        F.HipRandomForestSurrogate(model_params=params)


def test_class_surface_and_plugin_layout():
    import _baybe_layout as bl
    import baybe_amd
    from baybe_amd import plugin

    S = F.HipRandomForestSurrogate
    assert baybe_amd.HipRandomForestSurrogate is S and baybe_amd.make_baybe_forest_surrogate is plugin.make_baybe_forest_surrogate
    s = S()
    assert s.model_params == {} and s.device == 0 and not hasattr(s, "__dict__")
    assert (S.supports_transfer_learning, S.supports_multi_output, S.is_ensemble) == (False, False, True)
    assert not S.is_available
    with pytest.raises(IncompatibilityError, match="BoTorch"):
        s.to_botorch()
    from baybe_amd.exceptions import ModelNotTrainedError

    with pytest.raises(ModelNotTrainedError):
        s.posterior_mean_var(np.zeros((1, 1)))
    B = plugin.make_baybe_forest_surrogate(bl.Surrogate)
    b = B(model_params={"n_estimators": 3})
    assert isinstance(b, bl.Surrogate) and issubclass(B, F.HipForestSurrogateImpl) and not hasattr(b, "__dict__")
    assert b._searchspace is None and b._measurements_hash is None and B.is_ensemble and B.fit is F.HipForestSurrogateImpl.fit
    with pytest.raises(TypeError, match="invalid"):
        B(model_params={"n_estimators": 5.3})


def test_constant_targets_fit_one_leaf():
    """``catch_constant_targets``: one value, or a standard deviation (unbiased) below 1e-6 -> no forest, one leaf holding the mean."""
    x = np.arange(8.0).reshape(4, 2)
    for y in (np.array([3.5]), np.full(4, 2.0), 2.0 + 1e-7 * np.arange(4)):
        packed, model = F.fit_forest(x[: len(y)], y, {"n_estimators": 7})
        assert model is None and list(packed["offsets"]) == [0, 1] and packed["children_left"][0] == -1
        F.check_packed(packed, 2)
        P = of.traverse(packed, x)
        assert np.array_equal(P, np.full((1, 4), np.mean(y)))
        mean, var = of.moments(P)
        assert np.array_equal(var, np.zeros(4)) and np.array_equal(mean, P[0])
    assert not F.is_constant_target(np.array([0.0, 1e-5])) and F.is_constant_target(np.array([0.0, 1e-6]))
    pytest.importorskip("sklearn")
    packed, model = F.fit_forest(x, np.array([0.0, 1.0, 0.5, 2.0]), {"n_estimators": 3, "random_state": 0})
    assert model is not None and len(packed["offsets"]) == 4


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

    monkeypatch.setattr(F.HipForestSurrogateImpl, "fit", no_fit)
    space, obj, meas = _context()

    def rec(**kw):
        return HipBotorchRecommender(surrogate_model=F.HipRandomForestSurrogate(), **kw)

    hybrid = SearchSpace(space.discrete)
    hybrid.continuous = type("Cont", (), {"is_empty": False})()
    for call in (lambda r: r.recommend(2, hybrid, obj, meas), lambda r: r.acquisition_values(meas, hybrid, obj, meas)):
        with pytest.raises(NotImplementedError, match="non-GP"):
            call(rec())
    with pytest.raises(IncompatibilityError, match="[Rr]ow shards"):
        rec(shard=object())._setup_botorch_acqf(space, obj, meas)
    for name in ("qNEI", "qLogNEI", "qLogNEHVI", "qNEHVI", "qLogNParEGO"):
        with pytest.raises(IncompatibleAcquisitionFunctionError):
            rec(acquisition_function=name)._setup_botorch_acqf(space, obj, meas)
    pareto = ParetoObjective([NumericalTarget("y"), NumericalTarget("z")])
    with pytest.raises(IncompatibleSurrogateError, match="single-output"):
        rec()._setup_botorch_acqf(space, pareto, meas)

    class Transformed:
        name, minimize = "y", False
        transformation = type("BellTransformation", (), {})()

    with pytest.raises(IncompatibilityError):
        rec()._setup_botorch_acqf(space, SingleTargetObjective(Transformed()), meas)
    with pytest.raises(IncompatibilityError, match="exceeds 64"):  # the batch caps of the joint q'-batch kernels apply unchanged
        rec().recommend(65, space, obj, meas)
    with pytest.raises(IncompatibilityError, match="exceeds 16"):
        rec(acquisition_function="qUCB").recommend(17, space, obj, meas)
    with pytest.raises(AssertionError, match="fit"):  # (and what is not refused does reach the fit)
        rec()._setup_botorch_acqf(space, obj, meas)


def test_surrogate_fit_refusals_use_the_references_texts():
    s = F.HipRandomForestSurrogate()
    space, obj, meas = _context()
    with pytest.raises(IncompatibleSurrogateError, match="single-output surrogate in a 2-target multi-output context"):
        s.fit(space, ParetoObjective([NumericalTarget("y"), NumericalTarget("z")]), meas)
    tasks = type("Tasks", (), {"n_tasks": 2, "task_idx": 0, "comp_rep_columns": space.comp_rep_columns, "scaling_bounds": space.scaling_bounds})()
    with pytest.raises(ValueError, match=r"task parameters but the selected surrogate model type \(HipRandomForestSurrogate\)"):
        s.fit(tasks, obj, meas)
    bad = meas.copy()
    bad.loc[bad.index[0], "x0"] = np.nan
    with pytest.raises(ValueError, match="NaN among the training rows"):
        s.fit(space, obj, bad)


# ---- the condition on the fixtures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_every_greedy_step_of_every_case_clears_the_margin(name):
    """Winner minus the best DIFFERING score >= 1e-8 at every step of the greedy batches the GPU test runs (all MC kinds, with and
    without pending points): the device's 1e-9 deviations cannot change a pick, so the GPU test may skip nothing."""
    c = fc.case(name)
    P, Ptrain = oracle_predictions(name)
    idx = F.ensemble_member_indices(c["S"], P.shape[0], c["sampler"])
    best = of.best_f(Ptrain, c["sign"])
    for kind in fc.MC_KINDS:
        for k in (0, 1):
            pend = P[:, fc.pending_rows(c["N"], k)] if k else None
            batch = min(max(fc.BATCHES), c["N"])
            picks, values, margins = of.greedy(kind, P, idx, best, c["sign"], batch, pend)
            assert len(set(picks)) == batch and all(math.isfinite(v) for v in values)
            assert min(margins) >= MARGIN, (name, kind, k, margins)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_mixed_pending_block_leaves_the_candidate_its_say(sign):
    """63 pending points must not swamp the candidate, or the k = 63 scores of the GPU test would be one or two numbers that say
    nothing about the candidate's walk: under block "a" each of qLogEI, qSR, qUCB and qPSTD takes at least 100 distinct values among
    the 257 rows at S = 512; block "b" is "a" reversed with the best row in its last slot."""
    g = mixed()
    c = fc.MIXED
    P = g["pred"]
    idx = F.ensemble_member_indices(512, P.shape[0], c["sampler"])
    best = of.best_f(g["pred_train"], sign)
    a, b = fc.mixed_pending_rows(P, sign, "a"), fc.mixed_pending_rows(P, sign, "b")
    m = sign * of.moments(P)[0]
    assert len(a) == len(b) == 63 and len(set(a)) == 63 and np.array_equal(b[:-1], a[::-1][:-1]) and b[-1] == np.argmax(m)
    assert m[a].max() <= np.delete(m, a).min()
    for kind in ("qLogEI", "qSR", "qUCB", "qPSTD"):
        distinct = len(np.unique(of.scores(kind, P, P[:, a], idx, best, sign)))
        assert distinct >= 100, (kind, sign, distinct)


def test_every_greedy_step_of_the_mixed_forest_clears_the_margin():
    """The condition of ``test_every_greedy_step_of_every_case_clears_the_margin`` for the batches the GPU test runs on ``MIXED``."""
    g = mixed()
    c = dict(fc.MIXED, **fc.MIXED["greedy"])
    P = g["pred"]
    idx = F.ensemble_member_indices(c["S"], P.shape[0], c["sampler"])
    assert len(set(idx)) == 6 and {1, 3} <= set(idx)  # (both trees above the LDS budget are read)
    best = of.best_f(g["pred_train"], c["sign"])
    for kind in fc.MIXED_GREEDY_KINDS:
        for k in (0, 1):
            pend = P[:, fc.pending_rows(c["N"], k)] if k else None
            batch = max(fc.MIXED_BATCHES)
            picks, values, margins = of.greedy(kind, P, idx, best, c["sign"], batch, pend)
            assert len(set(picks)) == batch and all(math.isfinite(v) for v in values)
            assert min(margins) >= MARGIN, (kind, k, margins)
