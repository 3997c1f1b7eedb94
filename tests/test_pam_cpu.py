"""k-medoids without a GPU: the exact-order oracle (tests/_oracle_pam.py) against the reference's own medoids, and the host logic of
``baybe_amd.clustering`` (validation, refusals, random draws, candidate subsets, residency, plug-in class) with the device surface
doubled by the oracle (``OracleRows``).  tests/test_pam_gpu.py holds the kernels to the same oracle on the device."""

import copy
import pickle
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from attrs import define, field

import _baybe_layout as bl
import _oracle_pam as oracle
import _pam_cases as pc
from _baybe_shim import NumericalDiscreteParameter, SearchSpace
from _reference import reference_available, reference_baybe
from baybe_amd import clustering, plugin

GOLDEN = Path(__file__).resolve().parent / "golden" / "pam_reference_medoids.npz"
GENERIC = pc.generic_cases()
ALL = pc.all_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture()
def double(monkeypatch):
    """The oracle-backed stand-in for the device surface."""
    monkeypatch.setattr(clustering, "_rows_factory", oracle.OracleRows)
    oracle.OracleRows.instances.clear()
    return oracle.OracleRows


# ---- the oracle against the reference ------------------------------------------------------------------------------------------
def test_golden_covers_every_generic_case(golden):
    assert sorted(golden.files) == sorted(c.name for c in GENERIC)
    assert all(len(c.points()) >= 20 * c.k for c in GENERIC)


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: c.name)
def test_oracle_reproduces_the_reference_medoids_on_generic_points(case, golden):
    got = case.expected()
    if got.ties_met == 0:
        assert got.medoids == golden[case.name].tolist()


def test_ties_are_rare_on_generic_points():
    """A condition on the cases, not a tolerance: at most one generic case in ten may meet a bit-equal tie that decides something
    (such a case is held to the oracle only).  If this fails, choose other seeds (``_pam_cases.SEED_SHIFT``)."""
    tied = [c.name for c in GENERIC if c.expected().ties_met > 0]
    assert 10 * len(tied) <= len(GENERIC), tied


def test_golden_is_current_where_the_reference_imports(golden):
    reference_baybe()
    from baybe.utils.clustering_algorithms import KMedoids

    for case in GENERIC:
        np.random.seed(case.seed)
        got = KMedoids(n_clusters=case.k, max_iter=100, init="k-medoids++").fit(case.points())
        assert got.medoid_indices_.tolist() == golden[case.name].tolist(), case.name
        want = case.expected()
        if want.ties_met == 0:
            assert got.medoid_indices_.tolist() == want.medoids and got.labels_.tolist() == want.labels.tolist(), case.name
            # inertia_: the reference's |x|^2 + |y|^2 - 2 x.y form leaves sqrt(cancellation error), about |x| sqrt(eps) ~ 1e-7 for
            # points of norm below 10, where a medoid's distance to itself is exactly 0: k such terms
            assert got.n_iter_ == want.n_iter and abs(got.inertia_ - want.inertia) <= 1e-6 * case.k, case.name


def test_random_draws_consume_the_generator_like_the_reference():
    reference_baybe()
    from baybe.utils.clustering_algorithms import KMedoids

    X = np.random.default_rng(5).standard_normal((200, 3))
    for init in ("k-medoids++", "random"):
        np.random.seed(21)
        KMedoids(n_clusters=7, max_iter=100, init=init).fit(X)
        after_ref = np.random.random()
        np.random.seed(21)
        oracle.k_medoids(X, 7, 100, init)
        assert np.random.random() == after_ref
        rs_ref, rs_ours = np.random.RandomState(8), np.random.RandomState(8)
        KMedoids(n_clusters=7, max_iter=100, init=init, random_state=rs_ref).fit(X)
        oracle.k_medoids(X, 7, 100, init, rs_ours)
        assert rs_ref.random_sample() == rs_ours.random_sample()


def test_the_special_cases_are_what_their_names_say():
    X = pc._duplicates()
    pick = np.random.RandomState(pc.DUPLICATE_DRAW_SEED).choice(70, 6, replace=False)
    assert len(np.unique(X[pick], axis=0)) < 6, "the seed no longer draws two identical rows"
    by_name = {c.name: c for c in ALL}
    with pytest.warns(UserWarning, match=r"Cluster \d is empty! self.labels_\[self.medoid_indices_\[\d\]\] may not be labeled"):
        np.random.seed(pc.DUPLICATE_DRAW_SEED)
        got = oracle.k_medoids(X, 6, 100, "random")
    lab, _, _ = oracle.assign(X, pick)
    assert lab[pick].tolist() != list(range(6))  # in the first iteration a medoid lies outside its own (empty) cluster
    assert len(set(got.medoids)) == 6  # ... and the clustering recovers from it
    assert 1 in np.bincount(by_name["outlier-700x3-k3"].expected().labels).tolist()  # a one-member cluster
    assert np.bincount(by_name["outlier-700x3-k3"].expected().labels).max() > 256  # ... next to one spanning row tiles
    more = by_name["max-iter-1-needs-more"]
    assert oracle.k_medoids(more.points(), more.k, 100, random_state_=np.random.RandomState(more.seed)).n_iter >= 1  # (the index of
    # the last iteration run: a second one was needed)
    assert by_name["max-iter-0"].expected().n_iter == 0 and by_name["max-iter-0"].expected().first_costs is None


# ---- validation and refusals ----------------------------------------------------------------------------------------------------
BAD_CALLS = [
    (dict(n_clusters=0), "n_clusters should be a nonnegative integer. 0 was given"),
    (dict(n_clusters=None), "n_clusters should be a nonnegative integer. None was given"),
    (dict(n_clusters=2.0), "n_clusters should be a nonnegative integer. 2.0 was given"),
    (dict(n_clusters=2, max_iter=-1), "max_iter should be a nonnegative integer. -1 was given"),
    (dict(n_clusters=2, init="nearest"), "init needs to be one of the following: ['random', 'heuristic', 'k-medoids++', 'build', 'array-like']"),
    (dict(n_clusters=5), "The number of medoids (5) must be less than the number of samples 4."),
]


@pytest.mark.parametrize("kwargs,text", BAD_CALLS, ids=[t[:30] for _, t in BAD_CALLS])
def test_validation_errors_carry_the_reference_texts(kwargs, text, double):
    X = np.arange(8.0).reshape(4, 2)
    with pytest.raises(ValueError) as ours:
        clustering.k_medoids(X, **kwargs)
    assert text in str(ours.value)
    assert not double.instances  # refused before anything goes to the device
    if reference_available():
        reference_baybe()
        from baybe.utils.clustering_algorithms import KMedoids

        with pytest.raises(ValueError) as theirs:
            KMedoids(**kwargs).fit(X)
        assert " ".join(str(ours.value).split()) == " ".join(str(theirs.value).split())


REFUSED = [dict(init="heuristic"), dict(init="build"), dict(init=np.zeros((2, 2))), dict(method="pam"), dict(metric="manhattan"),
           dict(metric="precomputed")]


@pytest.mark.parametrize("kwargs", REFUSED, ids=lambda k: "-".join(f"{a}={type(b).__name__ if not isinstance(b, str) else b}" for a, b in k.items()))
def test_what_the_hip_path_leaves_out_is_refused(kwargs, double):
    with pytest.raises(ValueError, match="not available on the HIP path"):
        clustering.k_medoids(np.arange(8.0).reshape(4, 2), 2, **kwargs)
    assert not double.instances
    with pytest.raises(ValueError, match="not available on the HIP path"):
        clustering.HipPAMClusteringRecommender(model_params=kwargs).recommend(2, _space(levels=3))


# ---- the host logic on the double -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_host_logic_on_the_double_equals_the_oracle(case, double):
    """Everything above the device surface - the draws, the set-up on rows of distances, the iteration, the warnings' order, the
    subset - against the oracle's single function."""
    want = case.expected()
    with warnings.catch_warnings(record=True) as ours:
        warnings.simplefilter("always")
        np.random.seed(case.seed)
        if case.rows is None:
            med, labels, inertia, n_iter = clustering.k_medoids(case.points(), case.k, case.max_iter, case.init, case.random_state,
                                                                return_info=True)
        else:
            d = case.points().shape[1]
            dev = oracle.OracleRows(case.points(), np.zeros(d), np.ones(d))
            dev.select(case.subset())
            med, labels, inertia, n_iter = clustering._cluster(dev, case.k, case.max_iter, case.init, case.random_state)
    with warnings.catch_warnings(record=True) as theirs:
        warnings.simplefilter("always")
        np.random.seed(case.seed)
        oracle.k_medoids(case.candidates(), case.k, case.max_iter, case.init, case.random_state)
    assert [int(m) for m in med] == want.medoids and labels.tolist() == want.labels.tolist()
    assert inertia == want.inertia and n_iter == want.n_iter
    assert [(w.category, str(w.message)) for w in ours] == [(w.category, str(w.message)) for w in theirs]


def test_the_same_seed_gives_the_same_medoids_for_the_global_and_an_int_random_state(double):
    X = pc._normal(300, 5)()
    np.random.seed(77)
    a = clustering.k_medoids(X, 6)
    b = clustering.k_medoids(X, 6, random_state=77)
    np.random.seed(77)
    assert a == b == oracle.k_medoids(X, 6).medoids
    c = clustering.k_medoids(X, 6, init="random", random_state=np.random.RandomState(3))
    assert c == oracle.k_medoids(X, 6, init="random", random_state_=3).medoids


def test_warnings_are_the_reference_texts(double):
    from sklearn.exceptions import ConvergenceWarning

    more = {c.name: c for c in ALL}["max-iter-1-needs-more"]
    np.random.seed(more.seed)
    with pytest.warns(ConvergenceWarning) as rec:
        clustering.k_medoids(more.points(), more.k, 1)
    assert str(rec[0].message) == ("Maximum number of iteration reached before convergence. Consider increasing max_iter to improve "
                                   "the fit.")
    np.random.seed(pc.DUPLICATE_DRAW_SEED)
    with pytest.warns(UserWarning) as rec:
        clustering.k_medoids(pc._duplicates(), 6, init="random")
    k = int(str(rec[0].message).split()[1])
    assert str(rec[0].message) == (f"Cluster {k} is empty! self.labels_[self.medoid_indices_[{k}]] may not be labeled with its "
                                   f"corresponding cluster ({k}).")


# ---- the recommender ------------------------------------------------------------------------------------------------------------
@define
class NonPredictiveReplica(bl.PureRecommender):
    """Layout replica of ``NonPredictiveRecommender`` over the replica of ``PureRecommender`` (tests/_baybe_layout.py), as in
    tests/test_fps_cpu.py."""

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


def test_plugin_class_builds_on_the_base_layout(double):
    Rec = plugin.make_baybe_pam_recommender(NonPredictiveReplica, "DISCRETE")
    r = Rec()
    assert isinstance(r, NonPredictiveReplica) and isinstance(r, bl.PureRecommender) and isinstance(r, bl.RecommenderProtocol)
    assert Rec.compatibility == "DISCRETE" and (r.model_params, r.device) == ({"max_iter": 100, "init": "k-medoids++"}, 0)
    assert Rec().model_params is not r.model_params
    assert not Rec.is_available and Rec.is_available() is False  # no HIP device here
    with pytest.raises(TypeError):
        Rec(model_params={"n_init": 50})
    with pytest.raises(TypeError):
        Rec(model_params=3)
    space = _space()
    np.random.seed(4)
    rec = r.recommend(8, space)
    assert r.calls == ["NonPredictiveRecommender.recommend", "PureRecommender.recommend"]
    np.random.seed(4)
    want = oracle.k_medoids(_scaled(space), 8).medoids
    assert rec.index.tolist() == space.discrete.comp_rep.index[want].tolist() and len(rec) == 8


def test_resident_matrix_is_keyed_on_content_and_later_calls_send_positions(double):
    r = clustering.HipPAMClusteringRecommender()
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
    assert double.instances[0].selects[-1].tolist() == np.flatnonzero(keep).tolist()
    assert keep[exp.index.get_indexer(second.index)].all()
    np.random.seed(2)
    want = oracle.k_medoids(_scaled(space)[keep], 5).medoids  # statistics of the WHOLE subspace, candidates in their own order
    assert second.index.tolist() == exp.index[np.flatnonzero(keep)[want]].tolist()
    r.recommend(5, _space(levels=5))
    assert len(double.instances) == 2  # another content: another matrix


def test_stand_alone_recommender_refuses_and_warns_in_the_reference_words(double):
    from baybe_amd.exceptions import IncompatibleArgumentError, NotEnoughPointsLeftError, UnusedObjectWarning

    r = clustering.HipPAMClusteringRecommender({"max_iter": 3, "init": "random", "random_state": 5})
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
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = r.recommend(4, space)
        want = oracle.k_medoids(_scaled(space), 4, 3, "random", 5).medoids
    assert got.index.tolist() == space.discrete.comp_rep.index[want].tolist()


def test_copies_share_and_pickles_drop_the_device_state(double):
    r = clustering.HipPAMClusteringRecommender({"max_iter": 100, "init": "k-medoids++", "random_state": 1})
    r.recommend(3, _space())
    assert r._fps_cache is not None
    c = copy.deepcopy(r)
    assert c._fps_cache is r._fps_cache and c.model_params == r.model_params and c.model_params is not r.model_params and c == r
    p = pickle.loads(pickle.dumps(r))
    assert p._fps_cache is None and p == r
    assert p.recommend(3, _space()).index.tolist() == r.recommend(3, _space()).index.tolist()


def test_package_exports():
    import baybe_amd

    assert baybe_amd.k_medoids is clustering.k_medoids
    assert baybe_amd.HipPAMClusteringRecommender is clustering.HipPAMClusteringRecommender
    assert {"k_medoids", "HipPAMClusteringRecommender"} <= set(baybe_amd.__all__)


# ---- on the reference's own Campaign ---------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore")
def test_two_phase_campaign_starts_with_the_pam_recommender(double):
    reference_baybe()
    from baybe import Campaign
    from baybe.parameters import NumericalDiscreteParameter as RefParameter
    from baybe.recommenders import TwoPhaseMetaRecommender
    from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender
    from baybe.searchspace import SearchSpace as RefSpace
    from baybe.targets import NumericalTarget

    _, _, Bayes = plugin.make_baybe_classes()
    Pam = plugin.make_baybe_pam_recommender()
    initial = Pam()
    assert isinstance(initial, NonPredictiveRecommender) and Pam.compatibility.name == "DISCRETE"
    vals = np.arange(6) / 5.0
    space = RefSpace.from_product([RefParameter(f"x{i}", vals * (i + 1)) for i in range(3)])
    camp = Campaign(space, NumericalTarget("y").to_objective(), TwoPhaseMetaRecommender(initial_recommender=initial, recommender=Bayes()))
    np.random.seed(6)
    got = camp.recommend(8)
    exp = space.discrete.exp_rep
    assert len(got) == 8 and list(got.columns) == ["x0", "x1", "x2"] and got.index.isin(exp.index).all() and got.index.is_unique
    np.random.seed(6)
    want = oracle.k_medoids(oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float)), 8).medoids
    assert got.index.tolist() == exp.index[want].tolist()
    assert pd.DataFrame.equals(got, exp.loc[got.index])
    with pytest.raises(Exception, match="non-predictive recommenders cannot use this information"):
        initial.recommend(2, space, pending_experiments=exp.iloc[:1])
