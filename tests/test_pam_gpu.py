"""k-medoids on the device (csrc/bbh_pam.hip through baybe_amd.clustering) against the exact-order oracle (tests/_oracle_pam.py):
medoids and labels as lists, the first iteration's cost vector and the per-row distances BITWISE - the kernels are compiled without
contraction, take an IEEE square root and add in ascending position, so they must produce the bits of the numpy loops - inertia and
n_iter equal.  Generic-position cases are held to the reference's own medoids as well (tests/golden/pam_reference_medoids.npz)."""

import warnings
from pathlib import Path

import numpy as np
import pytest

import _oracle_pam as oracle
import _pam_cases as pc
from _baybe_shim import NumericalDiscreteParameter, SearchSpace

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "pam_reference_medoids.npz"
ALL = pc.all_cases() + [pc.LONG]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _device_rows(case):
    from baybe_amd import clustering

    d = case.points().shape[1]
    dev = clustering.DeviceRows(case.points(), np.zeros(d), np.ones(d))
    if case.rows is not None:
        dev.select(case.subset())
    return dev


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_device_clustering_equals_the_oracle(case, golden):
    from baybe_amd import clustering

    want = case.expected()
    dev = _device_rows(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the warnings' texts and order are host logic: tests/test_pam_cpu.py)
        np.random.seed(case.seed)
        med, labels, inertia, n_iter = clustering._cluster(dev, case.k, case.max_iter, case.init, case.random_state)
    assert [int(m) for m in med] == want.medoids
    assert labels.dtype == np.int32 and labels.tolist() == want.labels.tolist()
    assert inertia == want.inertia and n_iter == want.n_iter
    _, dist = dev.assign(med)
    assert np.array_equal(dist, want.dist), np.abs(dist - want.dist).max()
    if case.generic and want.ties_met == 0:
        assert want.medoids == golden[case.name].tolist()


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_first_iteration_costs_equal_the_oracle_bitwise(case):
    """One step from the oracle's own initial medoids: the cost of every row in its cluster, the updated medoids, the flags."""
    from baybe_amd import clustering

    P = case.candidates()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(case.seed)
        start = oracle.k_medoids(P, case.k, 0, case.init, case.random_state).medoids
    ref = oracle.OracleRows(P, np.zeros(P.shape[1]), np.ones(P.shape[1]))
    want_med, want_empty, want_changed = ref.step(start)
    dev = _device_rows(case)
    med, empty, changed = dev.step(np.asarray(start, dtype=np.int64))
    got, want = dev.costs(), ref.costs()
    live = ~np.isnan(want)  # (every row belongs to a non-empty cluster: all of them)
    assert live.all() and np.array_equal(got, want), np.abs(got - want).max()
    assert med.tolist() == want_med.tolist() and empty == want_empty and changed == want_changed
    rows = dev.dist_rows(np.asarray(start[:3], dtype=np.int64))
    assert np.array_equal(rows, ref.dist_rows(start[:3]))


def test_two_runs_under_one_seed_are_identical():
    from baybe_amd import clustering

    X = pc._normal(1000, 20)()
    runs = [clustering.k_medoids(X, 12, random_state=5, return_info=True) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2:] == runs[1][2:]
    np.random.seed(5)
    assert clustering.k_medoids(X, 12) == runs[0][0]


def _space(levels=6, dims=3):
    vals = np.arange(levels) / (levels - 1)
    return SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals * (i + 1)) for i in range(dims)])


def test_recommender_end_to_end_and_resident_matrix_reuse(monkeypatch):
    """``HipPAMClusteringRecommender().recommend(8, space)`` on a 6 x 6 x 6 product space returns the labels of the oracle's medoids; a
    second call on a shrunk candidate set uploads nothing again (call counter on the upload) and gathers the candidates' rows from
    the resident matrix (call counter on the prepare wrapper: one call per candidate set)."""
    from baybe_amd import clustering
    from baybe_amd.engine import HipGP

    uploads, prepares = [], []
    upload, prepare = clustering.DeviceRows._upload, HipGP.fps_prepare
    monkeypatch.setattr(clustering.DeviceRows, "_upload", lambda self, v: (uploads.append(1), upload(self, v))[1])
    monkeypatch.setattr(HipGP, "fps_prepare", lambda self, *a, **k: (prepares.append(a[-1] if len(a) > 3 else k.get("order")),
                                                                      prepare(self, *a, **k))[1])
    space = _space()
    exp, comp = space.discrete.exp_rep, space.discrete.comp_rep
    scaled = oracle.standard_scale(comp.to_numpy(dtype=float))
    r = clustering.HipPAMClusteringRecommender()
    assert r.is_available
    np.random.seed(3)
    first = r.recommend(8, space)
    np.random.seed(3)
    want = oracle.k_medoids(scaled, 8).medoids
    assert first.index.tolist() == comp.index[want].tolist() and first.equals(exp.loc[first.index])
    assert len(uploads) == 1 and all(p is None for p in prepares)
    n_prepared = len(prepares)
    keep = np.ones(len(exp), dtype=bool)
    keep[exp.index.get_indexer(first.index)] = False
    keep[1::4] = False
    np.random.seed(4)
    second = r.recommend(8, space.filtered(keep))
    assert len(uploads) == 1, "the resident matrix must be reused"
    assert len(prepares) == n_prepared + 1 and prepares[-1] is not None  # one gather of the candidates' rows, on the device
    np.random.seed(4)
    want = oracle.k_medoids(scaled[keep], 8).medoids
    assert second.index.tolist() == exp.index[np.flatnonzero(keep)[want]].tolist()


def test_argument_checks_of_the_entry_points_set_the_error():
    import torch

    from baybe_amd._lib import HipError
    from baybe_amd.engine import HipGP

    gp = HipGP(0)
    P = torch.zeros((2, 256), dtype=torch.float64, device="cuda")
    wide = torch.zeros((769, 256), dtype=torch.float64, device="cuda")
    idx = torch.zeros(3, dtype=torch.int64, device="cuda")
    starts = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(HipError, match="bbh_pam_dist_rows: bad arguments .*1 <= d <= 768"):
        gp.pam_dist_rows(wide, 10, idx)
    with pytest.raises(HipError, match="bbh_pam_dist_rows: bad arguments .*ld >= M"):
        gp.pam_dist_rows(P, 300, idx)
    with pytest.raises(HipError, match="bbh_pam_dist_rows: bad arguments .*1 <= T"):
        gp.pam_dist_rows(P, 10, idx[:0])
    with pytest.raises(HipError, match="bbh_pam_assign: bad arguments .*1 <= k <= M"):
        gp.pam_assign(P, 2, idx)
    with pytest.raises(HipError, match="bbh_pam_cost: bad arguments .*1 <= k <= M"):
        gp.pam_cost(P, 2, starts, starts, 3)
    with pytest.raises(HipError, match="bbh_pam_update: bad arguments .*1 <= k <= M"):
        gp.pam_update(torch.zeros(2, dtype=torch.float64, device="cuda"), idx, 2, starts, idx)
    out = gp.pam_dist_rows(P, 10, torch.tensor([0, 10, -1], device="cuda"))  # rows out of range: NaN, nothing read out of bounds
    assert out[0].eq(0).all() and out[1:].isnan().all()
    gp.close()
