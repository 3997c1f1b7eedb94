"""k-means on the device (csrc/bbh_kmeans.hip through baybe_amd.clustering) against the numpy oracle (tests/_oracle_kmeans.py).

The device adds in another order than numpy (a 256-position tile in ascending position, tiles ascending), so centres are held to
1e-11 absolute and inertia to 1e-11 relative: ten times the bound of the oracle-against-scikit-learn test, for sums over at most
1e3 to 2e4 members of size O(1) - a bound from fp64 error analysis (n * 2^-53 * |x| ~ 2e4 * 1.1e-16 * 4 ~ 1e-11 in the worst
case, 1e-13 typically), not a measurement.  Labels, ``n_iter``, the winning restart and the selection are compared for identity
only where the oracle's own margins are far larger (``Result.clears()``; asserted for the generic cases in tests/test_kmeans_cpu.py)
or where its ties are bit-equal on exact sums (``Case.exact`` and ``Result.decidable()``).  Every figure is printed before it is
asserted."""

import warnings

import numpy as np
import pytest

import _kmeans_cases as kc
import _oracle_kmeans as oracle
from _baybe_shim import SearchSpace

pytestmark = pytest.mark.gpu

ALL = kc.all_cases()
CENTRE_TOL = 1e-11
INERTIA_TOL = 1e-11


def _device_rows(case):
    from baybe_amd import clustering

    d = case.points().shape[1]
    dev = clustering.DeviceRows(case.points(), np.zeros(d), np.ones(d))
    if case.rows is not None:
        dev.select(case.subset())
    return dev


def _fit(case, dev):
    from baybe_amd import clustering

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the warning's text is host logic: tests/test_kmeans_cpu.py)
        np.random.seed(case.seed)
        return clustering._kmeans_fit(dev, case.k, random_state=case.random_state, **case.kwargs())


def _check_valid(P, centres, labels, inertia, n_iter, selection, case, relocated):
    """What holds for a clustering whatever way its near-ties fell."""
    k = case.k
    assert centres.shape == (k, P.shape[1]) and np.isfinite(centres).all()
    assert labels.shape == (len(P),) and labels.min() >= 0 and labels.max() < k and 0 <= n_iter <= case.max_iter
    d2 = np.stack([oracle.d2_to(P, c) for c in centres], axis=1)
    own = d2[np.arange(len(P)), labels]
    if not relocated:  # every point sits with a nearest centre (to rounding: a strict stop keeps the labels of the pass before)
        assert (own <= d2.min(axis=1) * (1 + 1e-9) + 1e-300).all()
    assert abs(inertia - own.sum()) <= INERTIA_TOL * max(own.sum(), 1e-300) or inertia == own.sum()
    pred = d2.argmin(axis=1)
    for c, j in enumerate(selection):
        if j == 0 and not (pred == c).any():
            continue  # a cluster without members
        assert d2[j, c] <= d2[j].min() * (1 + 1e-9) + 1e-300  # a member of its cluster ...
        assert d2[j, c] <= d2[pred == c, c].min(initial=np.inf) * (1 + 1e-9) + 1e-300  # ... and the nearest of them


def _compare(case, dev, got, want):
    centres, labels, inertia, n_iter, best = got
    selection = dev.kmeans_select(centres).tolist()
    err_c = float(np.abs(centres - want.centres).max())
    err_i = abs(inertia - want.inertia) / want.inertia if want.inertia > 0 else abs(inertia - want.inertia)
    print(f"{case.name}: centres {err_c:.3e} inertia {err_i:.3e} n_iter {n_iter}/{want.n_iter} best {best}/{want.best} "
          f"margins {want.min_margin:.1e} {want.min_seed_margin:.1e} {want.min_stop_gap:.1e} {want.min_inertia_gap:.1e} "
          f"ties {want.ties_met} empties {want.empties_met}")
    if want.clears() or (case.exact and want.decidable()):
        assert labels.dtype == np.int32 and labels.tolist() == want.labels.tolist()
        assert n_iter == want.n_iter and best == want.best and selection == want.selection
        assert err_c <= CENTRE_TOL and err_i <= INERTIA_TOL
        if case.exact:
            assert np.array_equal(centres, want.centres)
    else:
        _check_valid(case.candidates(), centres, labels, inertia, n_iter, selection, case, want.empties_met > 0)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_device_clustering_equals_the_oracle(case):
    dev = _device_rows(case)
    _compare(case, dev, _fit(case, dev), case.expected())


def test_the_long_case():
    case = kc.LONG
    want = case.expected()
    assert want.clears(), "the long case needs another seed"
    dev = _device_rows(case)
    _compare(case, dev, _fit(case, dev), want)


# (N, d, k, restarts): the edges of the 256-position tile; 48 restarts share a tile at this k * d: one tile exactly, and one more;
# three restart tiles of 21; the one-restart form with its centres streamed in chunks of 8
ONE_ITERATION = [(255, 3, 12, 3), (256, 3, 12, 3), (257, 3, 12, 3), (130, 3, 3, 48), (130, 3, 3, 49), (1000, 20, 12, 50), (40, 768, 11, 2),
                 (130, 16, 6, 3), (130, 17, 6, 3)]


@pytest.mark.parametrize("N,d,k,R", ONE_ITERATION, ids=lambda v: str(v))
def test_one_lloyd_iteration_from_given_centres(N, d, k, R):
    from baybe_amd import clustering

    P = kc._normal(N, d)()
    rng = np.random.default_rng(N + d + k + R)
    centres = np.stack([P[rng.choice(N, k, replace=False)] + 0.01 * rng.standard_normal((k, d)) for _ in range(R)])
    dev = clustering.DeviceRows(P, np.zeros(d), np.ones(d))
    rt, chunks = dev.gp.kmeans_plan(d, k, R)
    assert (rt, chunks > 1) == {3: (R, False), 48: (48, False), 49: (48, False), 50: (21, False), 2: (1, True)}[R]
    m = oracle.Margins()
    want = [oracle.assign(P, C, m) for C in centres]
    assert m.label >= 1e-10 and m.ties == 0  # a condition on the fixture
    dev.kmeans_begin(centres=centres)
    same, shift = dev.kmeans_step(list(range(R)))
    sums, counts = dev.kmeans_sums()
    assert not same.any()
    worst = 0.0
    for r in range(R):
        labels, dmin = want[r]
        new, want_sums, want_counts = oracle.update(P, labels, dmin, centres[r])
        assert dev.kmeans_labels(r).tolist() == labels.tolist() and counts[r].tolist() == want_counts.tolist()
        if (want_counts > 0).all():
            worst = max(worst, float(np.abs(sums[r] - want_sums).max()), float(np.abs(dev.kmeans_centres(r) - new).max()),
                        abs(shift[r] - np.sum((new - centres[r]) ** 2)) / shift[r])
    print(f"{(N, d, k, R)}: worst deviation {worst:.3e}")
    assert worst <= CENTRE_TOL


SEEDING = [(257, 3, 12, 3), (1000, 20, 12, 50), (130, 3, 3, 50), (40, 768, 11, 2), (65, 3, 65, 2), (300, 5, 1, 3)]


@pytest.mark.parametrize("N,d,k,R", SEEDING, ids=lambda v: str(v))
def test_the_seeding_alone_equals_the_oracle(N, d, k, R):
    from baybe_amd import clustering

    P = kc._normal(N, d)()
    T = 2 + int(np.log(k))
    U = np.random.RandomState(N + k).random_sample((R, 1 + (k - 1) * T))
    first = oracle.first_centres(N, U[:, 0])
    m = oracle.Margins()
    want = np.stack([oracle.kpp(P, k, int(first[r]), U[r, 1:], m) for r in range(R)])
    print(f"{(N, d, k, R)}: seed margin {m.seed:.3e} ties {m.ties}")
    assert m.seed >= 1e-10 and m.ties == 0  # a condition on the fixture
    dev = clustering.DeviceRows(P, np.zeros(d), np.ones(d))
    assert dev.kmeans_seed(first, U[:, 1:], k).tolist() == want.tolist()


def test_two_runs_under_one_seed_are_identical():
    from baybe_amd import clustering

    X = kc._normal(1000, 20)()
    runs = [clustering.k_means(X, 12, n_init=50, max_iter=1000, random_state=5, return_info=True) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2:] == runs[1][2:]
    np.random.seed(5)
    assert np.array_equal(clustering.k_means(X, 12, n_init=50, max_iter=1000), runs[0][0])


def _space():
    """A search space given as a table of seeded points: a product space is all mathematical ties (rows that share coordinates), on
    which no decision can be compared."""
    import pandas as pd

    return SearchSpace.from_dataframe(pd.DataFrame(kc._normal(216, 3)(), columns=["x0", "x1", "x2"]))


def test_recommender_end_to_end_and_resident_matrix_reuse(monkeypatch):
    """``HipKMeansClusteringRecommender().recommend(8, space)`` (the reference's defaults: 50 restarts) on seeded points returns the
    labels of the oracle's selection; a second call on a shrunk candidate set uploads nothing again (call counter on the upload) and
    gathers the candidates' rows from the resident matrix (call counter on the prepare wrapper: one call per candidate set)."""
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
    r = clustering.HipKMeansClusteringRecommender()
    assert r.is_available and r.model_params == {"max_iter": 1000, "n_init": 50}
    np.random.seed(3)
    first = r.recommend(8, space)
    np.random.seed(3)
    want = oracle.k_means(scaled, 8, n_init=50, max_iter=1000)
    assert want.clears()
    assert first.index.tolist() == comp.index[want.selection].tolist() and first.equals(exp.loc[first.index])
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
    want = oracle.k_means(scaled[keep], 8, n_init=50, max_iter=1000)
    assert want.clears()
    assert second.index.tolist() == exp.index[np.flatnonzero(keep)[want.selection]].tolist()


def test_argument_checks_of_the_entry_points_set_the_error():
    import torch

    from baybe_amd._lib import HipError
    from baybe_amd.engine import HipGP

    gp = HipGP(0)
    P = torch.zeros((2, 256), dtype=torch.float64, device="cuda")
    wide = torch.zeros((769, 256), dtype=torch.float64, device="cuda")
    idx = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    U = torch.zeros((2, 6), dtype=torch.float64, device="cuda")
    C3 = torch.zeros((2, 3, 2), dtype=torch.float64, device="cuda")
    rid = torch.arange(2, dtype=torch.int32, device="cuda")
    labels = torch.full((2, 300), -1, dtype=torch.int32, device="cuda")
    d2 = torch.zeros((2, 300), dtype=torch.float64, device="cuda")
    with pytest.raises(HipError, match="bbh_kmeans_plan: bad arguments .*1 <= d <= 768"):
        gp.kmeans_plan(769, 3, 2)
    with pytest.raises(HipError, match="bbh_kmeans_plan: bad arguments .*R >= 1"):
        gp.kmeans_plan(2, 3, 0)
    with pytest.raises(HipError, match="bbh_kmeans_seed: bad arguments .*1 <= d <= 768"):
        gp.kmeans_seed(wide, 10, idx, U, 3)
    with pytest.raises(HipError, match="bbh_kmeans_seed: bad arguments .*ld >= M"):
        gp.kmeans_seed(P, 300, idx, U, 3)
    with pytest.raises(HipError, match="bbh_kmeans_seed: bad arguments .*1 <= k <= M"):
        gp.kmeans_seed(P, 2, idx, U, 3)
    with pytest.raises(HipError, match="bbh_kmeans_seed: bad arguments .*1 <= T <= 32"):
        gp.kmeans_seed(P, 10, idx, U, 33)
    with pytest.raises(HipError, match="bbh_kmeans_pass: bad arguments .*1 <= k <= M"):
        gp.kmeans_pass(P, 2, C3, rid, labels, d2)
    with pytest.raises(HipError, match="bbh_kmeans_pass: bad arguments .*ld >= M"):
        gp.kmeans_pass(P, 300, C3, rid, labels, d2)
    out = gp.kmeans_pass(P, 10, C3, rid, labels, d2)
    out["work_f64"] = out["work_f64"][:3]
    with pytest.raises(HipError, match="bbh_kmeans_pass: bad arguments .*the work arrays need"):
        gp.kmeans_pass(P, 10, C3, rid, labels, d2, out)
    with pytest.raises(HipError, match="bbh_kmeans_select: bad arguments .*1 <= k <= M"):
        gp.kmeans_select(labels[0, :2], d2[0, :2], 3)
    sel = gp.kmeans_select(labels[0, :10], d2[0, :10], 3)  # every point sits in cluster 0: the others have no members
    assert sel.tolist() == [0, 0, 0]
    gp.close()
