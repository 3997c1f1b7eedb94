"""Gaussian mixture clustering without a GPU: the numpy oracle (tests/_oracle_gmm.py) against scikit-learn's own ``GaussianMixture``
and the reference's selection, the conditions on the fixtures, and the host logic of ``baybe_amd.clustering`` (draws, stopping,
restart choice, validation, refusals, warnings, candidate subsets, residency, plug-in class) with the device surface doubled by the
oracle (``OracleRows``).  tests/test_gmm_gpu.py holds the kernels to the same oracle on the device."""

import copy
import pickle
import re
import sys
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from attrs import define, field

import _baybe_layout as bl
import _gmm_cases as gc
import _oracle_gmm as oracle
from _baybe_shim import NumericalDiscreteParameter, SearchSpace
from _reference import reference_baybe
from baybe_amd import clustering, plugin
from baybe_amd.clustering import gaussian_mixture  # noqa: F401  (the feature under test: without it nothing here runs)

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from make_gmm_golden import reference_selection  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "gmm_reference_selection.npz"
GENERIC = gc.generic_cases()
ALL = gc.all_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture()
def double(monkeypatch):
    """The oracle-backed stand-in for the device surface."""
    monkeypatch.setattr(clustering, "_rows_factory", oracle.OracleRows)
    monkeypatch.setattr(oracle.OracleRows, "gmm_group", None)
    oracle.OracleRows.instances.clear()
    return oracle.OracleRows


# ---- the oracle against scikit-learn, and the conditions on the fixtures --------------------------------------------------------
@pytest.mark.parametrize("case", GENERIC, ids=lambda c: c.name)
def test_generic_cases_clear_the_conditions(case):
    """Conditions on the fixtures, not tolerances.  A case that fails here gets another seed (``_gmm_cases.SEED_SHIFT``), not a
    looser test."""
    r = case.expected()
    g = r.margins
    print(case.name, g.label, g.stop, g.restart, g.cond, g.flagged, g.init_ok)
    assert g.label >= 1e-6 and g.stop >= 1e-6 and g.restart >= 1e-9 and g.cond <= 1e4 and not g.flagged
    assert g.init_ok and r.clears()
    assert case.tolerances()["same"]  # the tile order takes the same decisions


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: c.name)
def test_oracle_equals_scikit_learn_on_generic_points(case, golden):
    mixture = pytest.importorskip("sklearn.mixture")
    X = case.points()
    np.random.seed(case.seed)
    ref = mixture.GaussianMixture(n_components=case.k, **case.kwargs()).fit(X)
    ref_labels = ref.predict(X)
    ref_selection = reference_selection(ref, X)
    after_ref = np.random.random()
    np.random.seed(case.seed)
    got = oracle.gaussian_mixture(X, case.k, **case.kwargs())
    assert np.random.random() == after_ref  # the global generator is in the same state after fit plus selection
    assert got.labels.tolist() == ref_labels.tolist() and got.n_iter == ref.n_iter_ and got.converged == ref.converged_
    worst = max(abs(got.lower_bound - ref.lower_bound_), np.abs(got.weights - ref.weights_).max(), np.abs(got.means - ref.means_).max(),
                np.abs(got.covariances - ref.covariances_).max())
    print(case.name, worst)
    assert worst <= 1e-12
    assert got.selection == ref_selection == golden[case.name].tolist()
    assert abs(float(golden[case.name + ":lower_bound"]) - ref.lower_bound_) <= 1e-12


def test_golden_covers_every_generic_case_and_the_oracle_reproduces_it(golden):
    assert sorted(golden.files) == sorted([c.name for c in GENERIC] + [c.name + ":lower_bound" for c in GENERIC])
    for case in GENERIC:
        want = case.expected()
        assert want.selection == golden[case.name].tolist(), case.name
        assert abs(want.lower_bound - float(golden[case.name + ":lower_bound"])) <= 1e-12, case.name


def test_the_special_cases_are_what_their_names_say():
    by_name = {c.name: c for c in ALL}
    assert by_name["max-iter-0"].expected().n_iter == 0 and by_name["max-iter-0"].expected().lower_bound == -np.inf
    assert by_name["max-iter-1"].expected().n_iter == 1 and not by_name["max-iter-1"].expected().converged
    singletons = by_name["edge-65x3-k65"].expected()
    assert np.bincount(singletons.labels).tolist() == [1] * 65 and sorted(singletons.selection) == list(range(65))
    assert np.allclose(singletons.covariances, 1e-6 * np.eye(3), rtol=0, atol=1e-15)
    flagged = by_name["edge-reg0-singletons-65x3-k65"].expected()
    assert isinstance(flagged, ValueError) and str(flagged) == oracle.ILL_DEFINED
    assert by_name["edge-40x64-k2"].expected().margins.cond > 1e4  # fewer members than columns: reg_covar carries the factor
    assert len(np.unique(by_name["duplicates"].points(), axis=0)) < len(by_name["duplicates"].points())
    assert by_name["init-random-from-data"].expected().lowers.shape == (2,)
    assert [c.n_init for c in GENERIC if c.n_init != 1] == [3, 3]
    assert gc.LONG.expected().clears(), "the long case needs another seed"


# ---- validation and refusals ----------------------------------------------------------------------------------------------------
BAD_CALLS = [
    (dict(n_components=0), "The 'n_components' parameter of GaussianMixture must be an int in the range [1, inf). Got 0 instead."),
    (dict(n_components=2.0), "The 'n_components' parameter of GaussianMixture must be an int in the range [1, inf). Got 2.0 instead."),
    (dict(n_components=2, tol=-1.0), "The 'tol' parameter of GaussianMixture must be a float in the range [0.0, inf). Got -1.0 instead."),
    (dict(n_components=2, reg_covar=-1.0), "The 'reg_covar' parameter of GaussianMixture must be a float in the range [0.0, inf). "
                                           "Got -1.0 instead."),
    (dict(n_components=2, max_iter=-1), "The 'max_iter' parameter of GaussianMixture must be an int in the range [0, inf). Got -1 instead."),
    (dict(n_components=2, n_init=0), "The 'n_init' parameter of GaussianMixture must be an int in the range [1, inf). Got 0 instead."),
    (dict(n_components=2, covariance_type="banana"), "The 'covariance_type' parameter of GaussianMixture must be a str among {'full', "
                                                     "'tied', 'diag', 'spherical'}. Got 'banana' instead."),
    (dict(n_components=2, init_params="nearest"), "The 'init_params' parameter of GaussianMixture must be a str among {'kmeans', "
                                                  "'random', 'random_from_data', 'k-means++'}. Got 'nearest' instead."),
    (dict(n_components=5), "Expected n_samples >= n_components but got n_components = 5, n_samples = 4"),
]


def _set_order_free(text):
    """scikit-learn prints a set of options in hash order: the options sorted."""
    return re.sub(r"\{([^}]*)\}", lambda m: "{" + ", ".join(sorted(m.group(1).split(", "))) + "}", " ".join(text.split()))


@pytest.mark.parametrize("kwargs,text", BAD_CALLS, ids=[f"{i}-{t[4:20]}" for i, (_, t) in enumerate(BAD_CALLS)])
def test_validation_errors_carry_the_scikit_learn_texts(kwargs, text, double):
    X = np.arange(8.0).reshape(4, 2)
    with pytest.raises(ValueError) as ours:
        clustering.gaussian_mixture(X, **kwargs)
    assert str(ours.value) == text
    assert not double.instances  # refused before anything goes to the device
    mixture = pytest.importorskip("sklearn.mixture")
    with pytest.raises(ValueError) as theirs:
        mixture.GaussianMixture(**kwargs).fit(X)
    assert _set_order_free(str(ours.value)) == _set_order_free(str(theirs.value))


def test_fewer_than_two_samples_are_refused_in_the_scikit_learn_words(double):
    with pytest.raises(ValueError) as ours:
        clustering.gaussian_mixture(np.zeros((1, 3)), 1)
    assert str(ours.value) == "Found array with 1 sample(s) (shape=(1, 3)) while a minimum of 2 is required by GaussianMixture."
    assert not double.instances
    mixture = pytest.importorskip("sklearn.mixture")
    with pytest.raises(ValueError) as theirs:
        mixture.GaussianMixture(1).fit(np.zeros((1, 3)))
    assert str(theirs.value) == str(ours.value)


REFUSED = [dict(covariance_type="diag"), dict(covariance_type="tied"), dict(covariance_type="spherical"), dict(init_params="random"),
           dict(weights_init=np.array([0.5, 0.5])), dict(means_init=np.zeros((2, 2))), dict(precisions_init=np.stack([np.eye(2)] * 2)),
           dict(warm_start=True)]


@pytest.mark.parametrize("kwargs", REFUSED, ids=lambda k: next(iter(k)) + "-" + str(next(iter(k.values())))[:9].split("\n")[0])
def test_what_the_hip_path_leaves_out_is_refused(kwargs, double):
    with pytest.raises(ValueError, match="not available on the HIP path"):
        clustering.gaussian_mixture(np.arange(8.0).reshape(4, 2), 2, **kwargs)
    with pytest.raises(ValueError, match="not available on the HIP path"):
        clustering.HipGaussianMixtureClusteringRecommender(model_params=kwargs).recommend(2, _space(levels=3))
    assert not double.instances


def test_more_than_64_columns_are_refused(double):
    with pytest.raises(ValueError, match="at most 64 columns"):
        clustering.gaussian_mixture(np.zeros((3, 65)), 2)
    with pytest.raises(ValueError, match="at most 65535 components, got 65536"):
        clustering.gaussian_mixture(np.zeros((65537, 1)), 65536)
    assert not double.instances


# ---- the host logic on the double -----------------------------------------------------------------------------------------------
def _fit_on_double(case):
    np.random.seed(case.seed)
    if case.rows is None:
        out = clustering.gaussian_mixture(case.points(), case.k, random_state=case.random_state, return_info=True, **case.kwargs())
        dev = oracle.OracleRows.instances[-1]
    else:  # a candidate subset of a resident matrix
        d = case.points().shape[1]
        dev = oracle.OracleRows(case.points(), np.zeros(d), np.ones(d))
        dev.select(case.subset())
        w, mu, cov, lower, n_iter, converged, _ = clustering._gmm_fit(dev, case.k, random_state=case.random_state, **case.kwargs())
        out = (w, mu, cov, dev.gmm_labels(), lower, n_iter, converged)
    return out + (clustering._gmm_select(dev).tolist(),)


@pytest.mark.parametrize("case", [c for c in ALL if c.n_init > 1], ids=lambda c: c.name)
def test_one_restart_per_group_gives_the_same_fit(case, double, monkeypatch):
    monkeypatch.setattr(oracle.OracleRows, "gmm_group", 1)
    _check_host_logic(case)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_host_logic_on_the_double_equals_the_oracle(case, double):
    """Everything above the device surface - the draws of all restarts up front, the groups of running restarts, the stopping rule,
    the restart choice, the warnings, the selection - against the oracle's single function."""
    _check_host_logic(case)


def _check_host_logic(case):
    want = case.expected()
    if case.raises:
        with pytest.raises(ValueError) as err:
            _fit_on_double(case)
        assert str(err.value) == str(want) == clustering._ILL_DEFINED
        return
    with warnings.catch_warnings(record=True) as ours:
        warnings.simplefilter("always")
        w, mu, cov, labels, lower, n_iter, converged, selection = _fit_on_double(case)
        after = np.random.random()
    with warnings.catch_warnings(record=True) as theirs:
        warnings.simplefilter("always")
        np.random.seed(case.seed)
        oracle.gaussian_mixture(case.candidates(), case.k, random_state_=case.random_state, **case.kwargs())
        assert np.random.random() == after
    assert np.array_equal(w, want.weights) and np.array_equal(mu, want.means) and np.array_equal(cov, want.covariances)
    assert labels.tolist() == want.labels.tolist() and lower == want.lower_bound
    assert (n_iter, converged, selection) == (want.n_iter, want.converged, want.selection)
    assert [(w.category, str(w.message)) for w in ours] == [(w.category, str(w.message)) for w in theirs]


def test_both_warnings_are_the_scikit_learn_texts(double):
    mixture = pytest.importorskip("sklearn.mixture")
    X = gc._normal(300, 5)()
    with pytest.warns(clustering.ConvergenceWarning) as rec:
        clustering.gaussian_mixture(X, 6, max_iter=1, random_state=5)
    with pytest.warns(clustering.ConvergenceWarning) as theirs:
        mixture.GaussianMixture(6, max_iter=1, random_state=5).fit(X)
    assert [str(w.message) for w in rec] == [str(w.message) for w in theirs] == [clustering._NOT_CONVERGED]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        clustering.gaussian_mixture(X, 6, max_iter=0, random_state=5)  # no iteration: no warning
    same = np.full((9, 3), 0.25)
    with pytest.warns(clustering.ConvergenceWarning) as rec:
        clustering.gaussian_mixture(same, 3, n_init=2, random_state=1)
    with pytest.warns(clustering.ConvergenceWarning) as theirs:
        mixture.GaussianMixture(3, n_init=2, random_state=1).fit(same)
    distinct = "Number of distinct clusters (1) found smaller than n_clusters (3). Possibly due to duplicate points in X."
    assert [str(w.message) for w in rec] == [str(w.message) for w in theirs]
    assert [str(w.message) for w in rec].count(distinct) == 2  # per restart


def test_the_flagged_restart_raises_the_scikit_learn_error(double):
    mixture = pytest.importorskip("sklearn.mixture")
    X = gc._normal(65, 3)()
    with pytest.raises(ValueError) as ours:
        clustering.gaussian_mixture(X, 65, reg_covar=0.0, random_state=1)
    with pytest.raises(ValueError) as theirs:
        mixture.GaussianMixture(65, reg_covar=0.0, random_state=1).fit(X)
    assert " ".join(str(ours.value).split()) == " ".join(str(theirs.value).split())


class _Scripted:
    """A device double whose restarts follow scripted lower bounds."""

    def __init__(self, script):
        self.script, self.m, self.d, self.at, self.predicted = script, 10, 2, [0] * len(script), None

    def gmm_begin(self, k, reg_covar, idx=None):
        return np.full(len(self.script), k), np.zeros(len(self.script), dtype=np.int64), len(self.script)

    def gmm_step(self, active, base):
        out = [self.script[r][self.at[r]] for r in active]
        for r in active:
            self.at[r] += 1
        return np.array(out), np.zeros(len(active), dtype=np.int64)

    def gmm_predict(self, r):
        self.predicted = r

    def gmm_result(self, r):
        return np.ones(1), np.zeros((1, 2)), np.eye(2)[None]


def test_restart_choice_takes_the_first_of_the_largest_lower_bounds(monkeypatch):
    monkeypatch.setattr(clustering, "_kpp_positions", lambda dev, k, R, rs: np.zeros((R, k), dtype=np.int64))
    script = [[-3.0, -2.0, -2.0], [-5.0, -1.5, -1.5004], [-3.0, -1.5, -1.5004], [-9.0, -9.0]]
    dev = _Scripted(script)
    *_, lower, n_iter, converged, best = clustering._gmm_fit(dev, 1, n_init=4, init_params="k-means++", random_state=0)
    assert (lower, n_iter, converged, best, dev.predicted) == (-1.5004, 3, True, 1, 1)  # restart 2 ends on the same bound: not strictly larger
    dev = _Scripted([[-3.0, -2.0], [-1.0, -0.5]])
    with pytest.warns(clustering.ConvergenceWarning, match="Best performing initialization did not converge"):
        *_, lower, n_iter, converged, best = clustering._gmm_fit(dev, 1, n_init=2, max_iter=2, init_params="k-means++", random_state=0)
    assert (lower, n_iter, converged, best) == (-0.5, 2, False, 1)


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


def _table(n=216, seed=0):
    """A search space given as a table of seeded points (a product space is all mathematical ties)."""
    return SearchSpace.from_dataframe(pd.DataFrame(gc._normal(n, 3, seed)(), columns=["x0", "x1", "x2"]))


def _scaled(space):
    return oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float))


def test_plugin_class_builds_on_the_base_layout(double):
    Rec = plugin.make_baybe_gmm_recommender(NonPredictiveReplica, "DISCRETE")
    r = Rec()
    assert isinstance(r, NonPredictiveReplica) and isinstance(r, bl.PureRecommender) and isinstance(r, bl.RecommenderProtocol)
    assert Rec.compatibility == "DISCRETE" and (r.model_params, r.device) == ({}, 0)
    assert Rec().model_params is not r.model_params
    assert not Rec.is_available and Rec.is_available() is False  # no HIP device here
    with pytest.raises(TypeError):
        Rec(model_params={"verbose": 1})
    with pytest.raises(TypeError):
        Rec(model_params=3)
    space = _table()
    np.random.seed(4)
    rec = r.recommend(8, space)
    assert r.calls == ["NonPredictiveRecommender.recommend", "PureRecommender.recommend"]
    np.random.seed(4)
    want = oracle.gaussian_mixture(_scaled(space), 8).selection
    assert rec.index.tolist() == space.discrete.comp_rep.index[want].tolist() and len(rec) == 8


def test_fewer_rows_than_the_batch_size_when_a_component_is_empty(double):
    """Identical candidates: every point goes to one component, the others have no members and yield no row - as in the reference."""
    space = SearchSpace.from_dataframe(pd.DataFrame(np.vstack([np.full((8, 2), 0.25), [[0.5, 0.75]]]), columns=["x0", "x1"]))
    r = clustering.HipGaussianMixtureClusteringRecommender()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(2)
        got = r.recommend(3, space)
        np.random.seed(2)
        want = oracle.gaussian_mixture(_scaled(space), 3)
    assert len(np.unique(want.labels)) < 3 and len(got) == len(want.selection) < 3
    assert got.index.tolist() == space.discrete.comp_rep.index[want.selection].tolist()


def test_resident_matrix_is_keyed_on_content_and_later_calls_send_positions(double):
    r = clustering.HipGaussianMixtureClusteringRecommender({"n_init": 2})
    space = _table()
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
    want = oracle.gaussian_mixture(_scaled(space)[keep], 5, n_init=2).selection  # statistics of the WHOLE subspace
    assert second.index.tolist() == exp.index[np.flatnonzero(keep)[want]].tolist()
    r.recommend(5, _table(seed=1))
    assert len(double.instances) == 2  # another content: another matrix


def test_stand_alone_recommender_refuses_and_warns_in_the_reference_words(double):
    from baybe_amd.exceptions import IncompatibleArgumentError, NotEnoughPointsLeftError, UnusedObjectWarning

    r = clustering.HipGaussianMixtureClusteringRecommender({"max_iter": 3, "random_state": 5})
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
    with pytest.raises(ValueError, match="The 'max_iter' parameter of GaussianMixture must be an int in the range"):
        clustering.HipGaussianMixtureClusteringRecommender({"max_iter": -1}).recommend(2, space)


def test_copies_share_and_pickles_drop_the_device_state(double):
    r = clustering.HipGaussianMixtureClusteringRecommender({"n_init": 2, "random_state": 1})
    space = _table()
    r.recommend(3, space)
    assert r._fps_cache is not None
    c = copy.deepcopy(r)
    assert c._fps_cache is r._fps_cache and c.model_params == r.model_params and c.model_params is not r.model_params and c == r
    p = pickle.loads(pickle.dumps(r))
    assert p._fps_cache is None and p == r
    np.random.seed(3)
    a = p.recommend(3, space).index.tolist()
    np.random.seed(3)
    assert a == r.recommend(3, space).index.tolist()


def test_package_exports():
    import baybe_amd

    assert baybe_amd.gaussian_mixture is clustering.gaussian_mixture
    assert baybe_amd.HipGaussianMixtureClusteringRecommender is clustering.HipGaussianMixtureClusteringRecommender
    assert {"gaussian_mixture", "HipGaussianMixtureClusteringRecommender"} <= set(baybe_amd.__all__)
    assert clustering.HipGaussianMixtureClusteringRecommender().model_params == {}


# ---- on the reference's own Campaign ---------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore")
def test_two_phase_campaign_starts_with_the_gmm_recommender(double):
    reference_baybe()
    from baybe import Campaign
    from baybe.parameters import NumericalDiscreteParameter as RefParameter
    from baybe.recommenders import TwoPhaseMetaRecommender
    from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender
    from baybe.searchspace import SearchSpace as RefSpace
    from baybe.targets import NumericalTarget

    _, _, Bayes = plugin.make_baybe_classes()
    GMM = plugin.make_baybe_gmm_recommender()
    initial = GMM()
    assert isinstance(initial, NonPredictiveRecommender) and GMM.compatibility.name == "DISCRETE" and initial.model_params == {}
    vals = np.arange(6) / 5.0
    space = RefSpace.from_product([RefParameter(f"x{i}", vals * (i + 1)) for i in range(3)])
    camp = Campaign(space, NumericalTarget("y").to_objective(), TwoPhaseMetaRecommender(initial_recommender=initial, recommender=Bayes()))
    np.random.seed(6)
    got = camp.recommend(8)
    exp = space.discrete.exp_rep
    assert 1 <= len(got) <= 8 and list(got.columns) == ["x0", "x1", "x2"] and got.index.isin(exp.index).all() and got.index.is_unique
    np.random.seed(6)
    want = oracle.gaussian_mixture(oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float)), 8).selection
    assert got.index.tolist() == exp.index[want].tolist()
    assert pd.DataFrame.equals(got, exp.loc[got.index])
    with pytest.raises(Exception, match="non-predictive recommenders cannot use this information"):
        initial.recommend(2, space, pending_experiments=exp.iloc[:1])
