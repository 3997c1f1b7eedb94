"""k-means without a GPU: the numpy oracle (tests/_oracle_kmeans.py) against scikit-learn's own ``KMeans`` and the reference's
selection, the margin conditions on the fixtures, and the host logic of ``baybe_amd.clustering`` (draws, stopping, restart choice,
validation, refusals, warnings, candidate subsets, residency, plug-in class) with the device surface doubled by the oracle
(``OracleRows``).  tests/test_kmeans_gpu.py holds the kernels to the same oracle on the device."""

import copy
import pickle
import sys
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from attrs import define, field

import _baybe_layout as bl
import _kmeans_cases as kc
import _oracle_kmeans as oracle
from _baybe_shim import NumericalDiscreteParameter, SearchSpace
from _reference import reference_baybe
from baybe_amd import clustering, plugin

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from make_kmeans_golden import reference_selection  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "kmeans_reference_selection.npz"
GENERIC = kc.generic_cases()
ALL = kc.all_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture()
def double(monkeypatch):
    """The oracle-backed stand-in for the device surface."""
    monkeypatch.setattr(clustering, "_rows_factory", oracle.OracleRows)
    oracle.OracleRows.instances.clear()
    return oracle.OracleRows


# ---- the oracle against scikit-learn, and the conditions on the fixtures --------------------------------------------------------
@pytest.mark.parametrize("case", GENERIC, ids=lambda c: c.name)
def test_generic_cases_clear_the_margin_conditions(case):
    """Conditions on the fixtures, not tolerances: every decision of the oracle has a margin orders of magnitude above fp64
    summation error.  A case that fails here gets another seed (``_kmeans_cases.SEED_SHIFT``), not a looser test."""
    r = case.expected()
    print(case.name, r.min_margin, r.min_seed_margin, r.min_select_margin, r.min_stop_gap, r.min_inertia_gap, r.ties_met, r.empties_met)
    assert r.min_margin >= 1e-10 and r.min_seed_margin >= 1e-10 and r.min_select_margin >= 1e-10
    assert r.min_stop_gap >= 1e-6 and r.min_inertia_gap >= 1e-9
    assert r.ties_met == 0 and r.empties_met == 0 and r.clears()


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: c.name)
def test_oracle_equals_scikit_learn_on_generic_points(case, golden):
    cluster = pytest.importorskip("sklearn.cluster")
    X = case.points()
    np.random.seed(case.seed)
    ref = cluster.KMeans(n_clusters=case.k, max_iter=case.max_iter, n_init=case.n_init).fit(X)
    after_ref = np.random.random()
    np.random.seed(case.seed)
    got = oracle.k_means(X, case.k, **case.kwargs())
    assert np.random.random() == after_ref  # the global generator is in the same state
    assert got.labels.tolist() == ref.labels_.tolist() and got.n_iter == ref.n_iter_
    assert np.abs(got.centres - ref.cluster_centers_).max() <= 1e-12
    assert abs(got.inertia - ref.inertia_) <= 1e-12 * ref.inertia_
    assert got.selection == reference_selection(ref, X) == golden[case.name].tolist()


def test_golden_covers_every_generic_case_and_the_oracle_reproduces_it(golden):
    assert sorted(golden.files) == sorted(c.name for c in GENERIC)
    for case in GENERIC:
        assert case.expected().selection == golden[case.name].tolist(), case.name


def test_the_special_cases_are_what_their_names_say():
    by_name = {c.name: c for c in ALL}
    X = kc._int_duplicates()
    pick = np.random.RandomState(kc.DUPLICATE_DRAW_SEED).choice(70, 6, replace=False)
    assert len(np.unique(X[pick], axis=0)) < 6, "the seed no longer draws two identical rows"
    drawn = by_name["exact-duplicates-random-identical-draw"].expected()
    assert drawn.seeds[0].tolist() == pick.tolist() and drawn.empties_met >= 1 and drawn.decidable()
    assert all(by_name[n].expected().ties_met > 0 and by_name[n].expected().decidable() for n in
               ("exact-grid-5^3-k5", "exact-grid-5^3-k5-random", "exact-duplicates-k6"))
    assert all(np.array_equal(c.points(), np.round(c.points() * 4) / 4) for c in kc.exact_cases())  # sums are exact
    assert by_name["max-iter-0"].expected().n_iter == 0 and by_name["max-iter-1"].expected().n_iter == 1
    more = by_name["max-iter-1"]
    np.random.seed(more.seed)
    assert oracle.k_means(more.points(), more.k, n_init=3).n_iter > 1  # one iteration was not enough
    assert by_name["init-random-auto"].expected().seeds.shape == (10, 6) and by_name["n-init-auto"].expected().seeds.shape == (1, 6)
    with pytest.warns(oracle.ConvergenceWarning, match=r"Number of distinct clusters \(1\) found smaller than n_clusters \(3\)"):
        oracle.k_means(np.full((9, 3), 0.25), 3, random_state_=1)


# ---- validation and refusals ----------------------------------------------------------------------------------------------------
BAD_CALLS = [
    (dict(n_clusters=0), "The 'n_clusters' parameter of KMeans must be an int in the range [1, inf). Got 0 instead."),
    (dict(n_clusters=None), "The 'n_clusters' parameter of KMeans must be an int in the range [1, inf). Got None instead."),
    (dict(n_clusters=2.0), "The 'n_clusters' parameter of KMeans must be an int in the range [1, inf). Got 2.0 instead."),
    (dict(n_clusters=2, n_init=0), "The 'n_init' parameter of KMeans must be a str among {'auto'} or an int in the range [1, inf). "
                                   "Got 0 instead."),
    (dict(n_clusters=2, n_init="many"), "The 'n_init' parameter of KMeans must be a str among {'auto'} or an int in the range [1, inf). "
                                        "Got 'many' instead."),
    (dict(n_clusters=2, max_iter=0), "The 'max_iter' parameter of KMeans must be an int in the range [1, inf). Got 0 instead."),
    (dict(n_clusters=2, tol=-1.0), "The 'tol' parameter of KMeans must be a float in the range [0.0, inf). Got -1.0 instead."),
    (dict(n_clusters=5), "n_samples=4 should be >= n_clusters=5."),
]


@pytest.mark.parametrize("kwargs,text", BAD_CALLS, ids=[f"{i}-{t[4:20]}" for i, (_, t) in enumerate(BAD_CALLS)])
def test_validation_errors_carry_the_scikit_learn_texts(kwargs, text, double):
    X = np.arange(8.0).reshape(4, 2)
    with pytest.raises(ValueError) as ours:
        clustering.k_means(X, **kwargs)
    assert str(ours.value) == text
    assert not double.instances  # refused before anything goes to the device
    cluster = pytest.importorskip("sklearn.cluster")
    with pytest.raises(ValueError) as theirs:
        cluster.KMeans(**kwargs).fit(X)
    assert " ".join(str(ours.value).split()) == " ".join(str(theirs.value).split())


REFUSED = [dict(init=np.zeros((2, 2))), dict(init=[[0.0, 0.0], [1.0, 1.0]]), dict(init=lambda X, k, rs: X[:k]), dict(algorithm="elkan")]


@pytest.mark.parametrize("kwargs", REFUSED, ids=["init-array", "init-list", "init-callable", "algorithm-elkan"])
def test_what_the_hip_path_leaves_out_is_refused(kwargs, double):
    with pytest.raises(ValueError, match="not available on the HIP path"):
        clustering.k_means(np.arange(8.0).reshape(4, 2), 2, **kwargs)
    with pytest.raises(ValueError, match="not available on the HIP path"):
        clustering.HipKMeansClusteringRecommender(model_params=kwargs).recommend(2, _space(levels=3))
    assert not double.instances


def test_sample_weights_and_unknown_values_are_refused(double):
    X = np.arange(8.0).reshape(4, 2)
    with pytest.raises(ValueError, match="Sample weights are not available on the HIP path"):
        clustering.k_means(X, 2, sample_weight=np.ones(4))
    with pytest.raises(ValueError, match="init needs to be 'k-means\\+\\+' or 'random'"):
        clustering.k_means(X, 2, init="nearest")
    with pytest.raises(ValueError, match="algorithm needs to be 'lloyd' or 'elkan'"):
        clustering.k_means(X, 2, algorithm="full")
    with pytest.raises(ValueError, match="at most 768 columns"):
        clustering.k_means(np.zeros((3, 769)), 2)
    assert not double.instances


# ---- the host logic on the double -----------------------------------------------------------------------------------------------
def _fit_on_double(case):
    np.random.seed(case.seed)
    if case.rows is None and case.max_iter >= 1:
        centres, labels, inertia, n_iter = clustering.k_means(case.points(), case.k, random_state=case.random_state, return_info=True,
                                                              **case.kwargs())
        dev = oracle.OracleRows.instances[-1]
    else:  # a candidate subset of a resident matrix; max_iter = 0 (refused by the public call, as in scikit-learn)
        d = case.points().shape[1]
        dev = oracle.OracleRows(case.points(), np.zeros(d), np.ones(d))
        dev.select(case.subset())
        centres, labels, inertia, n_iter, _ = clustering._kmeans_fit(dev, case.k, random_state=case.random_state, **case.kwargs())
    return centres, labels, inertia, n_iter, dev.kmeans_select(centres).tolist()


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_host_logic_on_the_double_equals_the_oracle(case, double):
    """Everything above the device surface - the draws of all restarts up front, the batch of running restarts, the stopping rules,
    the restart choice, the warning - against the oracle's single function."""
    want = case.expected()
    with warnings.catch_warnings(record=True) as ours:
        warnings.simplefilter("always")
        centres, labels, inertia, n_iter, selection = _fit_on_double(case)
    with warnings.catch_warnings(record=True) as theirs:
        warnings.simplefilter("always")
        np.random.seed(case.seed)
        oracle.k_means(case.candidates(), case.k, random_state_=case.random_state, **case.kwargs())
    assert np.array_equal(centres, want.centres) and labels.tolist() == want.labels.tolist()
    assert inertia == want.inertia and n_iter == want.n_iter and selection == want.selection
    assert [(w.category, str(w.message)) for w in ours] == [(w.category, str(w.message)) for w in theirs]


def test_the_draws_consume_the_generator_like_the_oracle(double):
    X = kc._normal(300, 5)()
    for init in ("k-means++", "random"):
        np.random.seed(21)
        clustering.k_means(X, 7, n_init=4, init=init)
        after = np.random.random()
        np.random.seed(21)
        oracle.k_means(X, 7, n_init=4, init=init)
        assert np.random.random() == after
        a, b = np.random.RandomState(8), np.random.RandomState(8)
        clustering.k_means(X, 7, n_init=4, init=init, random_state=a)
        oracle.k_means(X, 7, n_init=4, init=init, random_state_=b)
        assert a.random_sample() == b.random_sample()
    np.random.seed(77)
    c1 = clustering.k_means(X, 6, n_init=2)
    c2 = clustering.k_means(X, 6, n_init=2, random_state=77)
    assert np.array_equal(c1, c2)


def test_the_warning_is_the_scikit_learn_text(double):
    with pytest.warns(clustering.ConvergenceWarning) as rec:
        clustering.k_means(np.full((9, 3), 0.25), 3, random_state=1)
    assert str(rec[0].message) == "Number of distinct clusters (1) found smaller than n_clusters (3). Possibly due to duplicate points in X."
    cluster = pytest.importorskip("sklearn.cluster")
    with pytest.warns(clustering.ConvergenceWarning) as theirs:
        cluster.KMeans(n_clusters=3, random_state=1).fit(np.full((9, 3), 0.25))
    assert str(theirs[0].message) == str(rec[0].message)


def test_restart_choice_keeps_the_first_of_two_equal_clusterings():
    a = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    assert clustering._same_clustering(np.array([2, 2, 0, 0, 1], dtype=np.int32), a, 3)
    assert not clustering._same_clustering(np.array([0, 1, 1, 1, 2], dtype=np.int32), a, 3)
    assert clustering._same_clustering(a, np.array([0, 0, 0, 0, 2], dtype=np.int32), 3)  # scikit-learn's one-sided mapping
    for l1, l2 in ((np.array([2, 2, 0, 0, 1]), a), (np.array([0, 1, 1, 1, 2]), a), (a, np.array([0, 0, 0, 0, 2]))):
        assert clustering._same_clustering(l1, l2, 3) == oracle.same_clustering(l1, l2, 3)


# ---- the recommender ------------------------------------------------------------------------------------------------------------
@define
class NonPredictiveReplica(bl.PureRecommender):
    """Layout replica of ``NonPredictiveRecommender`` over the replica of ``PureRecommender`` (tests/_baybe_layout.py), as in
    tests/test_pam_cpu.py."""

    calls: list = field(factory=list, init=False, eq=False, repr=False)

    def recommend(self, batch_size, searchspace, objective=None, measurements=None, pending_experiments=None):
        if pending_experiments is not None:
            raise ValueError("replica: pending experiments refused")
        self.calls.append("NonPredictiveRecommender.recommend")
        return super().recommend(batch_size, searchspace, objective, measurements, None)

    def _recommend_with_discrete_parts(self, searchspace, batch_size, pending_experiments):
        candidates_exp, _ = searchspace.discrete.get_candidates()
        idxs = self._recommend_discrete(searchspace.discrete, candidates_exp, batch_size)
        return searchspace.discrete.exp_rep.loc[idxs, :]


def _space(levels=6, dims=3):
    vals = np.arange(levels) / (levels - 1)
    return SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals * (i + 1)) for i in range(dims)])


def _scaled(space):
    return oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float))


FAST = {"max_iter": 1000, "n_init": 4}


def test_plugin_class_builds_on_the_base_layout(double):
    Rec = plugin.make_baybe_kmeans_recommender(NonPredictiveReplica, "DISCRETE")
    r = Rec()
    assert isinstance(r, NonPredictiveReplica) and isinstance(r, bl.PureRecommender) and isinstance(r, bl.RecommenderProtocol)
    assert Rec.compatibility == "DISCRETE" and (r.model_params, r.device) == ({"max_iter": 1000, "n_init": 50}, 0)
    assert Rec().model_params is not r.model_params
    assert not Rec.is_available and Rec.is_available() is False  # no HIP device here
    with pytest.raises(TypeError):
        Rec(model_params={"verbose": 1})
    with pytest.raises(TypeError):
        Rec(model_params=3)
    space = _space()
    r = Rec(FAST)
    np.random.seed(4)
    rec = r.recommend(8, space)
    assert r.calls == ["NonPredictiveRecommender.recommend", "PureRecommender.recommend"]
    np.random.seed(4)
    want = oracle.k_means(_scaled(space), 8, **FAST).selection
    assert rec.index.tolist() == space.discrete.comp_rep.index[want].tolist() and len(rec) == 8


def test_resident_matrix_is_keyed_on_content_and_later_calls_send_positions(double):
    r = clustering.HipKMeansClusteringRecommender(FAST)
    space = _space()
    exp = space.discrete.exp_rep
    np.random.seed(1)
    first = r.recommend(5, space)
    assert len(double.instances) == 1
    keep = np.ones(len(exp), dtype=bool)
    keep[exp.index.get_indexer(first.index)] = False
    keep[::3] = False
    np.random.seed(2)
    second = r.recommend(5, space.filtered(keep))
    assert len(double.instances) == 1, "a shrunk candidate set must not upload the matrix again"
    assert double.instances[0].selects[-1].tolist() == np.flatnonzero(keep).tolist()  # positions only
    assert keep[exp.index.get_indexer(second.index)].all()
    np.random.seed(2)
    want = oracle.k_means(_scaled(space)[keep], 5, **FAST).selection  # statistics of the WHOLE subspace, candidates in their own order
    assert second.index.tolist() == exp.index[np.flatnonzero(keep)[want]].tolist()
    r.recommend(5, _space(levels=5))
    assert len(double.instances) == 2  # another content: another matrix


def test_stand_alone_recommender_refuses_and_warns_in_the_reference_words(double):
    from baybe_amd.exceptions import IncompatibleArgumentError, NotEnoughPointsLeftError, UnusedObjectWarning

    params = {"max_iter": 3, "n_init": 2, "init": "random", "random_state": 5}
    r = clustering.HipKMeansClusteringRecommender(params)
    space = _space(levels=3)
    with pytest.raises(IncompatibleArgumentError, match="non-predictive recommenders cannot use this information"):
        r.recommend(2, space, pending_experiments=space.discrete.exp_rep.iloc[:1])
    meas = space.discrete.exp_rep.iloc[:2].copy()
    meas["y"] = [0.0, 1.0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=Warning)
        warnings.simplefilter("error", category=UnusedObjectWarning)
        with pytest.raises(UnusedObjectWarning, match="does not utilize any training data"):
            r.recommend(2, space, measurements=meas)
        with pytest.raises(UnusedObjectWarning, match="does not consider any objectives"):
            r.recommend(2, space, objective=object())
    with pytest.raises(NotEnoughPointsLeftError, match="fewer than 28 possible data points"):
        r.recommend(28, space)
    with pytest.raises(ValueError, match="The 'max_iter' parameter of KMeans must be an int in the range"):
        clustering.HipKMeansClusteringRecommender({"max_iter": 0}).recommend(2, space)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = r.recommend(4, space)
        want = oracle.k_means(_scaled(space), 4, 2, 3, init="random", random_state_=5).selection
    assert got.index.tolist() == space.discrete.comp_rep.index[want].tolist()


def test_copies_share_and_pickles_drop_the_device_state(double):
    r = clustering.HipKMeansClusteringRecommender({"max_iter": 100, "n_init": 2, "random_state": 1})
    r.recommend(3, _space())
    assert r._fps_cache is not None
    c = copy.deepcopy(r)
    assert c._fps_cache is r._fps_cache and c.model_params == r.model_params and c.model_params is not r.model_params and c == r
    p = pickle.loads(pickle.dumps(r))
    assert p._fps_cache is None and p == r
    assert p.recommend(3, _space()).index.tolist() == r.recommend(3, _space()).index.tolist()


def test_package_exports():
    import baybe_amd

    assert baybe_amd.k_means is clustering.k_means
    assert baybe_amd.HipKMeansClusteringRecommender is clustering.HipKMeansClusteringRecommender
    assert {"k_means", "HipKMeansClusteringRecommender"} <= set(baybe_amd.__all__)
    assert clustering.HipKMeansClusteringRecommender().model_params == {"max_iter": 1000, "n_init": 50}


# ---- on the reference's own Campaign ---------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore")
def test_two_phase_campaign_starts_with_the_kmeans_recommender(double):
    reference_baybe()
    from baybe import Campaign
    from baybe.parameters import NumericalDiscreteParameter as RefParameter
    from baybe.recommenders import TwoPhaseMetaRecommender
    from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender
    from baybe.searchspace import SearchSpace as RefSpace
    from baybe.targets import NumericalTarget

    _, _, Bayes = plugin.make_baybe_classes()
    KMeans = plugin.make_baybe_kmeans_recommender()
    initial = KMeans(FAST)
    assert isinstance(initial, NonPredictiveRecommender) and KMeans.compatibility.name == "DISCRETE"
    assert KMeans().model_params == {"max_iter": 1000, "n_init": 50}
    vals = np.arange(6) / 5.0
    space = RefSpace.from_product([RefParameter(f"x{i}", vals * (i + 1)) for i in range(3)])
    camp = Campaign(space, NumericalTarget("y").to_objective(), TwoPhaseMetaRecommender(initial_recommender=initial, recommender=Bayes()))
    np.random.seed(6)
    got = camp.recommend(8)
    exp = space.discrete.exp_rep
    assert len(got) == 8 and list(got.columns) == ["x0", "x1", "x2"] and got.index.isin(exp.index).all() and got.index.is_unique
    np.random.seed(6)
    want = oracle.k_means(oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float)), 8, **FAST).selection
    assert got.index.tolist() == exp.index[want].tolist()
    assert pd.DataFrame.equals(got, exp.loc[got.index])
    with pytest.raises(Exception, match="non-predictive recommenders cannot use this information"):
        initial.recommend(2, space, pending_experiments=exp.iloc[:1])
