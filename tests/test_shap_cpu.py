"""Host side of the Shapley explanations (``baybe_amd.insights``): the weight matrix against exact rational arithmetic, the oracle
of tests/_oracle_shap.py against the permutation definition, group construction, every validation and refusal text, and the column
alignment of ``HipSHAPInsight.explain_target`` - the last ones over a numpy stand-in for the device engine."""

import itertools
import math
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import _oracle_shap as osh
import _shap_cases as sc
from baybe_amd import insights
from baybe_amd.exceptions import IncompatibilityError, IncompatibleExplainerError, NoMeasurementsError


# ---- W ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", range(1, 17))
def test_weights_against_rational_arithmetic(M):
    w = insights.shapley_weights(M)
    exact = [Fraction(math.factorial(s) * math.factorial(M - s - 1), math.factorial(M)) for s in range(M)]
    assert [Fraction(float(x)) for x in w] == [Fraction(float(e)) for e in exact]  # each weight is the correctly rounded quotient
    # in exact arithmetic: a row of W holds C(M - 1, s) entries +w[s] and as many -w[s]; the positive ones sum to 1
    assert sum(math.comb(M - 1, s) * e for s, e in enumerate(exact)) == 1
    W = insights.shapley_matrix(M)
    assert W.shape == (M, 1 << M)
    S = np.arange(1 << M)
    size = sum((S >> g) & 1 for g in range(M))
    for g in range(M):
        has = ((S >> g) & 1).astype(bool)
        assert np.array_equal(W[g, has], w[size[has] - 1]) and np.array_equal(W[g, ~has], -w[size[~has]])
        assert np.array_equal(np.sort(W[g, has]), np.sort(-W[g, ~has]))  # the row sums to 0 term by term
        assert abs(math.fsum(W[g])) <= 1e-15 and abs(math.fsum(W[g, has]) - 1.0) <= 1e-13


@pytest.mark.parametrize("M", range(1, 7))
def test_matrix_entries_against_fractions(M):
    W = insights.shapley_matrix(M)
    for g, S in itertools.product(range(M), range(1 << M)):
        k = bin(S).count("1")
        e = Fraction(math.factorial(k - 1) * math.factorial(M - k), math.factorial(M)) if (S >> g) & 1 else \
            -Fraction(math.factorial(k) * math.factorial(M - k - 1), math.factorial(M))
        assert W[g, S] == float(e), (M, g, S)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (1, 2, 3, 4))
def test_oracle_against_the_permutation_definition(M):
    rng = np.random.default_rng(M)
    v = rng.standard_normal((3, 1 << M))
    a, b = osh.subset_shapley(v, M), osh.permutation_shapley(v, M)
    assert np.abs(a - b).max() <= 1e-14 * np.abs(v).max() * (1 << M)
    assert np.abs(a - v @ insights.shapley_matrix(M).T).max() <= 1e-14 * np.abs(v).max() * (1 << M)
    assert np.abs(a.sum(axis=1) - (v[:, -1] - v[:, 0])).max() <= 1e-14 * np.abs(v).max() * (1 << M)  # efficiency


def test_oracle_composes_rows_and_keeps_ungrouped_columns():
    x, Bg = np.array([10.0, 11.0, 12.0, 13.0]), np.array([[0.0, 1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0]])
    rows = osh.compose_rows(x, Bg, np.array([1, -1, 0, 1]), 2)
    assert rows.shape == (4, 2, 4)
    assert np.array_equal(rows[0], Bg)
    assert np.array_equal(rows[1], [[0.0, 1.0, 12.0, 3.0], [4.0, 5.0, 12.0, 7.0]])  # feature 0 = column 2
    assert np.array_equal(rows[2], [[10.0, 1.0, 2.0, 13.0], [10.0, 5.0, 6.0, 13.0]])  # feature 1 = columns 0 and 3
    assert np.array_equal(rows[3], [[10.0, 1.0, 12.0, 13.0], [10.0, 5.0, 12.0, 13.0]])  # column 1 is the background's throughout
    # a linear f: phi_g = sum over the group's columns of c_j (x_j - mean_b b_j), exactly the textbook result
    coef = np.array([1.0, 2.0, 3.0, 4.0])
    v = osh.coalition_values(lambda r: r @ coef, x[None], Bg, np.array([1, -1, 0, 1]), 2)
    phi = osh.subset_shapley(v, 2)[0]
    dx = coef * (x - Bg.mean(axis=0))
    assert np.allclose(phi, [dx[2], dx[0] + dx[3]], rtol=1e-14)


def test_cases_are_what_they_say():
    for case in sc.CASES + [sc.COMPOSITE_CASE, sc.ICM_CASE]:
        c = case.build()
        assert c.X.shape == (case.R, case.d) and c.Bg.shape == (case.B, case.d) and c.Xt.shape == (case.n, case.d)
        assert set(case.groups.tolist()) - {-1} == set(range(case.M))
        if case.R >= 2:
            assert np.array_equal(c.X[0], c.Bg[0]) and np.array_equal(c.X[1], c.Xt[0])
        if case.R >= 17:
            assert np.array_equal(c.X[-1], c.X[3])
    assert sc.BY_ID["m5-rbf"].groups.tolist().count(1) == 3 and -1 in sc.BY_ID["m5-rbf"].groups
    assert {(c.kernel, c.scale) for c in sc.CASES if c.M == 5} == {(k, s) for k in sc.KINDS for s in (False, True)}


@pytest.mark.parametrize("case", [sc.BY_ID["n17"], sc.BY_ID["m5-matern52-os"], sc.COMPOSITE_CASE, sc.ICM_CASE], ids=lambda c: c.id)
def test_case_models_are_well_conditioned_and_efficient(case):
    om, ref = case.oracle_model(), case.reference()
    K = om.L @ om.L.T
    assert np.linalg.cond(K) <= 1e4
    c = case.build()
    if -1 not in case.groups:  # efficiency of the oracle: sum_g phi + base = f(x)
        assert np.abs(ref.phi.sum(axis=1) + ref.base - om.posterior(np.array(c.X))[0]).max() <= 16 * ref.tol_phi
    assert ref.tol_v > 0.0


# ---- groups -------------------------------------------------------------------------------------------------------------------------
def _space(with_indices=True, extra=()):
    return sc.StubSpace([sc.NumericalParameter("x", (0.0, 1.0)), sc.CategoricalParameter("c", ("a", "b", "c")),
                         sc.NumericalParameter("z", (0.0, 2.0))], with_indices=with_indices, extra_columns=extra)


@pytest.mark.parametrize("with_indices", (True, False))
def test_groups_in_the_experimental_representation(with_indices):
    groups, names = insights.feature_groups(_space(with_indices))
    assert names == ["x", "c", "z"] and groups.tolist() == [0, 1, 1, 1, 2] and groups.dtype == np.int32


def test_groups_in_the_computational_representation_and_ungrouped_columns():
    groups, names = insights.feature_groups(_space(), use_comp_rep=True)
    assert names == ["x", "c_a", "c_b", "c_c", "z"] and groups.tolist() == [0, 1, 2, 3, 4]
    groups, names = insights.feature_groups(_space(extra=("aux",)))
    assert names == ["x", "c", "z"] and groups.tolist() == [0, 1, 1, 1, 2, -1]


# ---- a numpy stand-in for the device engine ---------------------------------------------------------------------------------------------
class _Host:
    def __init__(self, a):
        self._a = a

    def cpu(self):
        return self

    def numpy(self):
        return self._a


class FakeEngine:
    """``shap_values`` by the oracle's formula for f(row) = row . coef + row[0] row[-1]."""

    _comm = None

    def __init__(self, d):
        self.coef = np.arange(1.0, d + 1.0)
        self.calls = []

    def f(self, rows):
        return rows @ self.coef + rows[:, 0] * rows[:, -1]

    def shap_values(self, X, background, groups, form="auto", want_v=False, n_groups=None):
        self.calls.append((np.array(X), np.array(background), np.array(groups), form, n_groups))
        v = osh.coalition_values(self.f, X, background, groups, n_groups)
        return _Host(osh.subset_shapley(v, n_groups)), float(v[0, 0]), None


class FakeSurrogate:
    def __init__(self, space):
        self._searchspace = space
        self.engine = FakeEngine(len(space.comp_rep_columns))

    def posterior_stats(self, *a, **k):
        raise NotImplementedError


def _frames():
    bg = pd.DataFrame({"x": [0.0, 1.0, 1.0, 0.0], "c": ["a", "b", "c", "b"], "z": [0.0, 2.0, 1.0, 0.5]})
    data = pd.DataFrame({"z": [1.5, 0.25], "note": ["p", "q"], "c": ["c", "a"], "x": [1.0, 0.0]})
    return bg, data


def test_explain_target_aligns_and_permutes_columns():
    space = _space()
    sur = FakeSurrogate(space)
    bg, data = _frames()
    ins = insights.HipSHAPInsight.from_surrogate(sur, bg)
    ex = ins.explain_target(0, data)
    assert ex.feature_names == ["z", "c", "x"] and ex.values.shape == (2, 3) and ex.shape == (2, 3)
    X, Bg, groups, form, M = sur.engine.calls[-1]
    assert M == 3 and form == "auto" and groups.tolist() == [0, 1, 1, 1, 2]
    assert np.array_equal(X, [[1.0, 0.0, 0.0, 1.0, 1.5], [0.0, 1.0, 0.0, 0.0, 0.25]])  # the comp rep in the search space's order
    assert np.array_equal(Bg, space.transform(bg).to_numpy())
    v = osh.coalition_values(sur.engine.f, X, Bg, groups, 3)
    phi = osh.subset_shapley(v, 3)  # features in group order x, c, z
    assert np.array_equal(ex.values, phi[:, [2, 1, 0]])
    assert np.array_equal(ex.base_values, np.full(2, v[0, 0]))
    assert ex.data.tolist() == [[1.5, "c", 1.0], [0.25, "a", 0.0]]
    # the background is the default data; explain() is the tuple over the targets
    (own,) = ins.explain()
    assert own.feature_names == ["x", "c", "z"] and own.values.shape == (4, 3)
    phi_t, base, names = insights.shapley_values(sur, bg, bg)
    assert names == ["x", "c", "z"] and np.array_equal(own.values, phi_t) and base == own.base_values[0]
    with pytest.raises(ValueError, match="must contain all columns that were used for the background data"):
        ins.explain_target(0, data.drop(columns="c"))


def test_comp_rep_insight_explains_columns():
    space = _space()
    sur = FakeSurrogate(space)
    bg, data = _frames()
    ins = insights.HipSHAPInsight.from_surrogate(sur, space.transform(bg), use_comp_rep=True, form="composed")
    ex = ins.explain_target(0, space.transform(data)[["z", "c_c", "c_b", "c_a", "x"]])
    assert ex.feature_names == ["z", "c_c", "c_b", "c_a", "x"] and ex.values.shape == (2, 5)
    X, Bg, groups, form, M = sur.engine.calls[-1]
    assert M == 5 and form == "composed" and groups.tolist() == [0, 1, 2, 3, 4]


def test_validation_and_refusal_texts():
    space = _space()
    sur = FakeSurrogate(space)
    bg, _ = _frames()
    with pytest.raises(ValueError, match="The provided background data set is empty."):
        insights.HipSHAPInsight.from_surrogate(sur, bg.iloc[:0])
    with pytest.raises(ValueError, match="only accepts the surrogate models of this package"):
        insights.HipSHAPInsight.from_surrogate(object(), bg)
    for name in ("PermutationExplainer", "LimeTabular", "Maple", "nonsense"):
        with pytest.raises(IncompatibleExplainerError, match="'KernelExplainer' and 'ExactExplainer'"):
            insights.HipSHAPInsight.from_surrogate(sur, bg, name)
    for name in insights.EXPLAINERS:
        assert len(insights.HipSHAPInsight.from_surrogate(sur, bg, explainer_cls=name).surrogates) == 1

    class Explainerish:  # a class is named by its __name__
        pass

    with pytest.raises(IncompatibleExplainerError, match="Explainerish"):
        insights.HipSHAPInsight.from_surrogate(sur, bg, Explainerish)

    class Campaign:
        measurements = pd.DataFrame()
        parameters = space.parameters
        searchspace = space

        def get_surrogate(self):
            return sur

    with pytest.raises(NoMeasurementsError, match="The campaign does not contain any measurements."):
        insights.HipSHAPInsight.from_campaign(Campaign())
    camp = Campaign()
    camp.measurements = bg.assign(t=[1.0, 2.0, 3.0, 4.0])
    ins = insights.HipSHAPInsight.from_campaign(camp)
    assert list(ins.background_data.columns) == ["x", "c", "z"]
    assert list(insights.HipSHAPInsight.from_campaign(camp, use_comp_rep=True).background_data.columns) == list(space.comp_rep_columns)
    with pytest.raises(TypeError, match="The provided recommender does not provide a surrogate model. 'HipSHAPInsight' needs a surrogate "
                                        "model and thus only works with model-based recommenders."):
        insights.HipSHAPInsight.from_recommender(object(), space, None, camp.measurements)

    class Recommender:
        def get_surrogate(self, searchspace, objective, measurements):
            assert searchspace is space and len(measurements) == 4
            return sur

    ins = insights.HipSHAPInsight.from_recommender(Recommender(), space, None, camp.measurements)
    assert list(ins.background_data.columns) == ["x", "c", "z"] and ins.explain()[0].values.shape == (4, 3)
    # row shards
    sur.engine._comm = (0, 2)
    with pytest.raises(IncompatibilityError, match="do not run over row shards"):
        insights.HipSHAPInsight.from_surrogate(sur, bg)
    sur.engine._comm = None
    # plots need the shap package
    try:
        import shap  # noqa: F401
    except Exception:  # noqa: BLE001
        with pytest.raises(ImportError, match="needs the optional package 'shap'"):
            ins.plot("bar")
        with pytest.raises(ImportError, match="needs the optional package 'shap'"):
            ins.explain()[0].to_shap()


def test_more_than_sixteen_features_are_refused_before_any_device_work():
    space = sc.StubSpace([sc.NumericalParameter(f"p{i}", (0.0, 1.0)) for i in range(17)])
    sur = FakeSurrogate(space)
    bg = pd.DataFrame(np.random.default_rng(0).random((3, 17)), columns=[f"p{i}" for i in range(17)])
    text = "stops at 16 features and 17 were requested.*use_comp_rep=False.*fewer parameters"
    with pytest.raises(IncompatibilityError, match=text):
        insights.HipSHAPInsight.from_surrogate(sur, bg)
    with pytest.raises(IncompatibilityError, match=text):
        insights.shapley_values(sur, bg, bg)
    assert sur.engine.calls == []
    # 16 one-hot columns + 1: too many in the comp rep, fine in the experimental one
    space = sc.StubSpace([sc.CategoricalParameter("c", tuple("abcdefghijklmnop")), sc.NumericalParameter("x", (0.0, 1.0))])
    sur = FakeSurrogate(space)
    bg = pd.DataFrame({"c": ["a", "b"], "x": [0.0, 1.0]})
    with pytest.raises(IncompatibilityError, match="stops at 16 features and 17 were requested"):
        insights.HipSHAPInsight.from_surrogate(sur, space.transform(bg), use_comp_rep=True)
    assert insights.HipSHAPInsight.from_surrogate(sur, bg).explain()[0].values.shape == (2, 2)
