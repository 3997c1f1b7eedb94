"""Farthest point sampling on the device (csrc/bbh_fps.hip through baybe_amd.sampling) against the exact-order oracle
(tests/_oracle_fps.py): picks as lists of ints, the per-pick squared distances BITWISE - the kernels' distance loops are compiled
without contraction and must produce the bits of a numpy loop over k.  Generic-position cases are held to the reference's own picks
as well (tests/golden/fps_reference_picks.npz)."""

import warnings
from pathlib import Path

import numpy as np
import pytest

import _fps_cases as fc
import _oracle_fps as oracle
from _baybe_shim import NumericalDiscreteParameter, SearchSpace

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "fps_reference_picks.npz"
ALL = fc.all_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _run(case):
    """(indices, d2) of the device path under the case's seed."""
    from baybe_amd import sampling

    np.random.seed(case.seed)
    if case.alive is None:
        return sampling.farthest_point_sampling(case.points(), case.n_samples, case.initialization, case.random_tie_break,
                                                return_distances=True)
    d = case.points().shape[1]
    dp = sampling.DevicePoints(case.points(), np.zeros(d), np.ones(d))
    return sampling._select(dp, case.n_samples, case.initialization, case.random_tie_break, case.mask())


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_device_picks_and_distances_equal_the_oracle(case, golden):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the all-identical cases warn on both sides)
        want_idx, want_d2 = case.expected()
        idx, d2 = _run(case)
    assert idx == want_idx
    assert np.array_equal(d2, want_d2), (d2 - want_d2)
    if case.generic:
        assert idx == golden[case.name].tolist()
    if case.alive is not None:
        assert case.mask()[idx].all(), "a masked row was returned"


def test_identical_points_take_the_warning_path_on_the_device():
    from baybe_amd import sampling

    with pytest.warns(UserWarning, match="All points are identical."):
        assert sampling.farthest_point_sampling(np.full((300, 5), 1.5), 7) == list(range(7))


@pytest.mark.parametrize("shape", [(65, 3), (1000, 20), (300, 33)], ids=str)
def test_prepared_matrix_and_ranking_equal_numpy(shape):
    """The resident matrix read back: numpy's (X - mean) / scale in np.lexsort order, bit for bit (IEEE division on the device, the
    ranking by stable sorts on the device)."""
    from baybe_amd import sampling

    rng = np.random.default_rng(sum(shape))
    X = rng.standard_normal(shape) * rng.uniform(0.5, 20.0, shape[1]) + rng.uniform(-3, 3, shape[1])
    X[:, 0] = np.round(X[:, 0])  # ties in the least significant key, resolved by the stability of the later sorts
    X[:, -1] = np.round(X[:, -1] / 5.0)  # ... and in the most significant one
    mean, scale = sampling.standard_scaling(X)
    dp = sampling.DevicePoints(X, mean, scale)
    scaled = (X - mean) / scale
    order = np.lexsort(tuple(scaled.T))
    assert np.array_equal(dp.order, order)
    assert np.array_equal(dp.points(), scaled[order])


def test_grid_scaling_on_the_device_equals_the_host():
    from baybe_amd import sampling

    levels, spans = fc.GRIDS["2x2x3x5x4"]
    axes = [np.linspace(0.0, spans[i], n) for i, n in enumerate(levels)]
    X = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(levels))
    mean, scale = sampling.standard_scaling(X)
    dp = sampling.DevicePoints(X, mean, scale)
    assert np.array_equal(dp.points(), oracle.standard_scale(X)[dp.order])


def test_the_greedy_pass_takes_more_columns_than_the_all_pairs_kernels():
    """768 columns are the limit of the all-pairs kernels' LDS tile alone: an index (or "random") start needs no farthest pair, and
    the greedy pass loops over any d."""
    from baybe_amd import sampling
    from baybe_amd._lib import HipError

    X = np.random.default_rng(769).standard_normal((40, 769))
    want, want_d2 = oracle.farthest_point_sampling(X, 5, [7, 2], False)
    idx, d2 = sampling.farthest_point_sampling(X, 5, [7, 2], False, return_distances=True)
    assert idx == want and np.array_equal(d2, want_d2)
    with pytest.raises(HipError, match="bbh_fps_farthest_pair: bad arguments.*d <= 768"):
        sampling.farthest_point_sampling(X, 5, "farthest", False)


def test_deterministic_mode_repeats_itself():
    from baybe_amd import sampling

    X = fc._grid([6] * 3)()
    runs = [sampling.farthest_point_sampling(X, 20, "farthest", False, return_distances=True) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])


def _space(levels=6, dims=3):
    vals = np.arange(levels) / (levels - 1)
    return SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals * (i + 1)) for i in range(dims)])


def test_recommender_end_to_end_and_resident_matrix_reuse(monkeypatch):
    """``HipFPSRecommender().recommend(8, space)`` on a 6 x 6 x 6 product space returns the labels of the oracle's picks; a second
    call on a shrunk candidate set prepares nothing again (call counter on the prepare entry point) and sends only a mask."""
    from baybe_amd import sampling
    from baybe_amd.engine import HipGP

    calls = []
    prepare = HipGP.fps_prepare
    monkeypatch.setattr(HipGP, "fps_prepare", lambda self, *a, **k: (calls.append(1), prepare(self, *a, **k))[1])
    space = _space()
    exp, comp = space.discrete.exp_rep, space.discrete.comp_rep
    scaled = oracle.standard_scale(comp.to_numpy(dtype=float))
    r = sampling.HipFPSRecommender()
    assert r.is_available
    first = r.recommend(8, space)
    want, _ = oracle.farthest_point_sampling(scaled, 8, "farthest", False)
    assert first.index.tolist() == comp.index[want].tolist() and first.equals(exp.loc[first.index])
    assert len(calls) == 2  # the unranked and the ranked matrix, once per search space
    keep = np.ones(len(exp), dtype=bool)
    keep[exp.index.get_indexer(first.index)] = False
    keep[1::4] = False
    second = r.recommend(8, space.filtered(keep))
    assert len(calls) == 2, "the resident matrix must be reused"
    want, _ = oracle.farthest_point_sampling(scaled, 8, "farthest", False, alive=keep)
    assert second.index.tolist() == comp.index[want].tolist() and keep[exp.index.get_indexer(second.index)].all()
    np.random.seed(5)
    third = sampling.HipFPSRecommender("random").recommend(8, space)
    np.random.seed(5)
    want, _ = oracle.farthest_point_sampling(scaled, 8, "random", True)
    assert third.index.tolist() == comp.index[want].tolist()


def test_argument_checks_of_the_entry_points_set_the_error():
    import torch

    from baybe_amd.engine import HipGP
    from baybe_amd._lib import HipError

    gp = HipGP(0)
    P = torch.zeros((2, 256), dtype=torch.float64, device="cuda")
    with pytest.raises(HipError, match="M >= 2"):
        gp.fps_farthest_pair(P, 1)
    with pytest.raises(HipError, match="start rank out of range"):
        gp.fps_greedy(P, 10, starts=[10])
    with pytest.raises(HipError, match="more picks requested than rows"):
        gp.fps_greedy(P, 3, starts=[0, 1], n_picks=2)
    gp.close()
    fresh = HipGP(0)  # the same handle, back from the pool: its selection ended when it went there
    with pytest.raises(HipError, match="no selection in progress"):
        fresh.fps_greedy(P, 3, n_picks=1)
    fresh.close()
