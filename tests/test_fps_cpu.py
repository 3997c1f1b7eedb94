"""Farthest point sampling without a GPU: the exact-order oracle (tests/_oracle_fps.py) against the reference's own picks, and the host
logic of ``baybe_amd.sampling`` (validation, random draws, rank / mask / label mapping, residency, plug-in class) with the device
surface doubled by the oracle (``OraclePoints``).  tests/test_fps_gpu.py holds the kernels to the same oracle on the device."""

import copy
import pickle
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from attrs import define, field

import _baybe_layout as bl
import _fps_cases as fc
import _oracle_fps as oracle
from _baybe_shim import NumericalDiscreteParameter, SearchSpace
from _reference import reference_available, reference_baybe
from baybe_amd import plugin, sampling

GOLDEN = Path(__file__).resolve().parent / "golden" / "fps_reference_picks.npz"
GENERIC = fc.generic_cases()
ALL = fc.all_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture()
def double(monkeypatch):
    """The oracle-backed stand-in for the device surface."""
    monkeypatch.setattr(sampling, "_points_factory", oracle.OraclePoints)
    oracle.OraclePoints.instances.clear()
    return oracle.OraclePoints


# ---- the oracle against the reference ------------------------------------------------------------------------------------------
def test_golden_covers_every_generic_case(golden):
    assert sorted(golden.files) == sorted(c.name for c in GENERIC)


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: c.name)
def test_oracle_reproduces_the_reference_picks_on_generic_points(case, golden):
    idx, d2 = case.expected()
    assert idx == golden[case.name].tolist()
    assert len(d2) == len(idx)


def test_golden_is_current_where_the_reference_imports(golden):
    reference_baybe()
    from baybe.utils.sampling_algorithms import farthest_point_sampling

    for case in GENERIC:
        np.random.seed(case.seed)
        got = farthest_point_sampling(case.points(), case.n_samples, case.initialization, case.random_tie_break)
        assert [int(i) for i in got] == golden[case.name].tolist(), case.name


def test_where_the_reference_matrix_is_asymmetric_at_its_maximum_the_start_pair_comes_out_mirrored():
    """d(a, b) and d(b, a) are one distance; the reference's GEMM-form matrix rounds them apart on this input, its argmax lands below
    the diagonal and the start is [b, a].  The contract resolves every tie in ranks - the smallest a first - so the picks are the
    same set with the first two exchanged (tests/_fps_cases.py: SEED_SHIFT)."""
    reference_baybe()
    from baybe.utils.sampling_algorithms import farthest_point_sampling

    N, d = fc.MIRRORED_START
    X = fc._normal(N, d, shift=0)()
    ref = [int(i) for i in farthest_point_sampling(X, 12, "farthest", False)]
    ours, _ = oracle.farthest_point_sampling(X, 12, "farthest", False)
    assert ours[:2] == ref[1::-1] and ours[2:] == ref[2:]


def test_random_draws_consume_the_generator_like_the_reference():
    """One randint for a "random" start, one choice per pick - also when a single row is tied - so the global generator is in the
    reference's state afterwards."""
    reference_baybe()
    from baybe.utils.sampling_algorithms import farthest_point_sampling

    X = np.random.default_rng(5).standard_normal((40, 3))
    for init in ("random", "farthest", [3, 1]):
        np.random.seed(21)
        farthest_point_sampling(X, 9, init, True)
        after_ref = np.random.random()
        np.random.seed(21)
        oracle.farthest_point_sampling(X, 9, init, True)
        assert np.random.random() == after_ref


# ---- scaling --------------------------------------------------------------------------------------------------------------------
def test_scaling_equals_sklearns_standard_scaler():
    sk = pytest.importorskip("sklearn.preprocessing")
    for name, (levels, spans) in fc.GRIDS.items():
        axes = [np.linspace(0.0, 1.0 if spans is None else spans[i], n) for i, n in enumerate(levels)]
        X = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(levels))
        mean, scale = sampling.standard_scaling(X)
        assert np.array_equal((X - mean) / scale, sk.StandardScaler().fit(X).transform(X)), name
    rng = np.random.default_rng(0)
    X = rng.standard_normal((500, 7)) * rng.uniform(0.1, 30.0, 7) + rng.uniform(-5, 5, 7)
    X[:, 3] = 0.1  # a constant column: scale 1
    mean, scale = sampling.standard_scaling(X)
    assert scale[3] == 1.0
    ours, theirs = (X - mean) / scale, sk.StandardScaler().fit(X).transform(X)
    assert np.all(np.abs(ours - theirs) <= 8 * np.spacing(np.abs(theirs)) + 1e-15)
    assert np.array_equal(ours, oracle.standard_scale(X))


# ---- validation and the warning path --------------------------------------------------------------------------------------------
BAD_CALLS = [
    (dict(points=np.zeros((4, 2)), n_samples=0), "The number of requested samples must be at least 1. Provided: n_samples=0."),
    (dict(points=np.zeros(4)), "The provided array must be two-dimensional but the given input had 1 dimensions."),
    (dict(points=np.zeros((0, 2))), "The provided array must contain at least one row."),
    (dict(points=np.zeros((4, 0))), "The provided input space must be at least one-dimensional."),
    (dict(points=np.zeros((4, 2)), initialization=[1, 1]), "must be unique but contains duplicates: {1}"),
    (dict(points=np.zeros((2, 2)), initialization=[0, 1, 2]), "(3) cannot be larger than the total number of points provided (2)."),
    (dict(points=np.zeros((4, 2)), initialization=[0, 7]), "(0 to 3) but contains out-of-bounds indices: [7]"),
    (dict(points=np.zeros((4, 2)), initialization="nearest"), "Unknown initialization type. Expected 'farthest', 'random', or a collection"),
    (dict(points=np.zeros((4, 2)), n_samples=5), "The number of requested samples (5) cannot be larger than the total number of points provided (4)."),
]


@pytest.mark.parametrize("kwargs,text", BAD_CALLS, ids=[t[:30] for _, t in BAD_CALLS])
def test_validation_errors_carry_the_reference_texts(kwargs, text, double):
    with pytest.raises(ValueError) as ours:
        sampling.farthest_point_sampling(**kwargs)
    assert text in str(ours.value)
    assert not double.instances  # refused before anything goes to the device
    if reference_available():
        reference_baybe()
        from baybe.utils.sampling_algorithms import farthest_point_sampling

        with pytest.raises(ValueError) as theirs:
            farthest_point_sampling(**kwargs)
        assert " ".join(str(ours.value).split()) == " ".join(str(theirs.value).split())


def test_identical_points_warn_and_return_the_first_rows(double):
    X = np.full((9, 3), 0.25)
    with pytest.warns(UserWarning, match="All points are identical."):
        assert sampling.farthest_point_sampling(X, 4) == [0, 1, 2, 3]
    with pytest.warns(UserWarning, match="All points are identical."):
        assert sampling.farthest_point_sampling(np.array([[1.0, 2.0]]), 1, "random") == [0]
    if reference_available():
        reference_baybe()
        from baybe.utils.sampling_algorithms import farthest_point_sampling

        with pytest.warns(UserWarning, match="All points are identical."):
            assert farthest_point_sampling(X, 4) == [0, 1, 2, 3]


# ---- the host logic on the double -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ALL if c.name != "planted-two-tile-segments"], ids=lambda c: c.name)
def test_host_logic_on_the_double_equals_the_oracle(case, double):
    """Everything above the device surface - ranks, masks, the draws from np.random, the mapping back to rows - against the oracle's
    single function.  (The 16700-row case is a kernel-path case: GPU test only.)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_idx, want_d2 = case.expected()
        np.random.seed(case.seed)
        if case.alive is None:
            idx, d2 = sampling.farthest_point_sampling(case.points(), case.n_samples, case.initialization, case.random_tie_break,
                                                       return_distances=True)
        else:
            d = case.points().shape[1]
            dp = oracle.OraclePoints(case.points(), np.zeros(d), np.ones(d))
            idx, d2 = sampling._select(dp, case.n_samples, case.initialization, case.random_tie_break, case.mask())
            assert case.mask()[idx].all()
    assert idx == want_idx and np.array_equal(d2, want_d2)


# ---- the plug-in class ----------------------------------------------------------------------------------------------------------
@define
class NonPredictiveReplica(bl.PureRecommender):
    """Layout replica of ``NonPredictiveRecommender`` over the replica of ``PureRecommender`` (tests/_baybe_layout.py): ``@define``
    without fields of its own, ``recommend`` refusing pending experiments and deferring to the parent, whose
    ``_recommend_with_discrete_parts`` extracts the candidates and calls ``_recommend_discrete`` (pure/base.py:248-310)."""

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


def test_plugin_class_builds_on_the_base_layout(double):
    Rec = plugin.make_baybe_fps_recommender(NonPredictiveReplica, "DISCRETE")
    r = Rec()
    assert isinstance(r, NonPredictiveReplica) and isinstance(r, bl.PureRecommender) and isinstance(r, bl.RecommenderProtocol)
    assert Rec.compatibility == "DISCRETE" and (r.initialization, r.random_tie_break, r.device) == ("farthest", False, 0)
    assert Rec("random").random_tie_break is True and Rec("random", random_tie_break=False).random_tie_break is False
    assert Rec(initialization="farthest", random_tie_break=True).random_tie_break is True
    assert not Rec.is_available and Rec.is_available() is False  # no HIP device here
    with pytest.raises(ValueError, match="not a valid FPSInitialization"):
        Rec("nearest")
    with pytest.raises(TypeError):
        Rec(random_tie_break=1)
    with pytest.raises(RuntimeError, match="deprecated"):
        Rec(allow_repeated_recommendations=True)  # the base's __attrs_post_init__ still runs
    space = _space()
    rec = r.recommend(8, space)
    assert r.calls == ["NonPredictiveRecommender.recommend", "PureRecommender.recommend"]
    scaled = oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float))
    want, _ = oracle.farthest_point_sampling(scaled, 8, "farthest", False)
    assert rec.index.tolist() == space.discrete.comp_rep.index[want].tolist() and len(rec) == 8


def test_resident_points_are_keyed_on_content_and_later_calls_send_a_mask(double):
    r = sampling.HipFPSRecommender()
    space = _space()
    exp = space.discrete.exp_rep
    first = r.recommend(5, space)
    assert len(double.instances) == 1
    keep = np.ones(len(exp), dtype=bool)
    keep[exp.index.get_indexer(first.index)] = False
    keep[::3] = False
    second = r.recommend(5, space.filtered(keep))
    assert len(double.instances) == 1, "a shrunk candidate set must not upload the matrix again"
    assert keep[exp.index.get_indexer(second.index)].all()
    scaled = oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float))  # statistics of the WHOLE subspace
    want, _ = oracle.farthest_point_sampling(scaled, 5, "farthest", False, alive=keep)
    assert second.index.tolist() == exp.index[want].tolist()
    other = _space(levels=5)
    r.recommend(5, other)
    assert len(double.instances) == 2  # another content: another matrix


def test_stand_alone_recommender_refuses_and_warns_in_the_reference_words(double):
    from baybe_amd.exceptions import IncompatibleArgumentError, NotEnoughPointsLeftError, UnusedObjectWarning

    r = sampling.HipFPSRecommender("random")
    space = _space(levels=3)
    with pytest.raises(IncompatibleArgumentError, match="non-predictive recommenders cannot use this information"):
        r.recommend(2, space, pending_experiments=space.discrete.exp_rep.iloc[:1])
    meas = space.discrete.exp_rep.iloc[:2].copy()
    meas["y"] = [0.0, 1.0]
    with pytest.warns(UnusedObjectWarning, match="does not utilize any training data"):
        r.recommend(2, space, measurements=meas)
    with pytest.warns(UnusedObjectWarning, match="does not consider any objectives"):
        r.recommend(2, space, objective=object())
    with pytest.raises(NotEnoughPointsLeftError, match="fewer than 28 possible data points"):
        r.recommend(28, space)
    np.random.seed(3)
    got = r.recommend(4, space)
    np.random.seed(3)
    want, _ = oracle.farthest_point_sampling(oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float)), 4, "random", True)
    assert got.index.tolist() == space.discrete.comp_rep.index[want].tolist()


def test_copies_share_and_pickles_drop_the_device_state(double):
    r = sampling.HipFPSRecommender()
    r.recommend(3, _space())
    assert r._fps_cache is not None
    c = copy.deepcopy(r)
    assert c._fps_cache is r._fps_cache and c.initialization == "farthest" and c == r
    p = pickle.loads(pickle.dumps(r))
    assert p._fps_cache is None and p == r
    assert p.recommend(3, _space()).index.tolist() == r.recommend(3, _space()).index.tolist()


def test_package_exports():
    import baybe_amd

    assert baybe_amd.farthest_point_sampling is sampling.farthest_point_sampling
    assert baybe_amd.HipFPSRecommender is sampling.HipFPSRecommender


# ---- on the reference's own Campaign ---------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore")
def test_two_phase_campaign_starts_with_the_fps_recommender(double):
    reference_baybe()
    from baybe import Campaign
    from baybe.parameters import NumericalDiscreteParameter as RefParameter
    from baybe.recommenders import TwoPhaseMetaRecommender
    from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender
    from baybe.searchspace import SearchSpace as RefSpace
    from baybe.targets import NumericalTarget

    _, _, Bayes = plugin.make_baybe_classes()
    Fps = plugin.make_baybe_fps_recommender()
    initial = Fps()
    assert isinstance(initial, NonPredictiveRecommender) and Fps.compatibility.name == "DISCRETE"
    vals = np.arange(6) / 5.0
    space = RefSpace.from_product([RefParameter(f"x{i}", vals * (i + 1)) for i in range(3)])
    camp = Campaign(space, NumericalTarget("y").to_objective(), TwoPhaseMetaRecommender(initial_recommender=initial, recommender=Bayes()))
    got = camp.recommend(8)
    exp = space.discrete.exp_rep
    assert len(got) == 8 and list(got.columns) == ["x0", "x1", "x2"] and got.index.isin(exp.index).all() and got.index.is_unique
    want, _ = oracle.farthest_point_sampling(oracle.standard_scale(space.discrete.comp_rep.to_numpy(dtype=float)), 8, "farthest", False)
    assert got.index.tolist() == exp.index[want].tolist()
    assert pd.DataFrame.equals(got, exp.loc[got.index])
    with pytest.raises(Exception, match="non-predictive recommenders cannot use this information"):
        initial.recommend(2, space, pending_experiments=exp.iloc[:1])
