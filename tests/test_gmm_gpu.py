"""Gaussian mixture clustering on the device (csrc/bbh_gmm.hip through baybe_amd.clustering) against the numpy oracle
(tests/_oracle_gmm.py).

Single steps from given inputs are held to bounds from fp64 error analysis, not to measurements:

* one M-step: ``nk``, means and covariances within 1e-11 absolute (``n * 2^-53 * |x|^2`` for n <= 1000 and ``|x|^2 <= 16``, times a
  few); the counts of a one-hot source are exact.
* one precision factor: ``max |P^T Sigma P - I| <= 8 d 2^-53 cond(Sigma)``, ``logdet`` against the oracle within the same bound.
* one E-step from parameters with cond <= 1e2: ``lp`` and ``log_resp`` within 1e-10 absolute (``d * 2^-53 * cond * q`` with d = 64
  and q ~ 130), labels identical where the fixture's label gap is >= 1e-6, the lower bound within 1e-11.

Whole fits pass errors through up to 100 EM iterations, so their tolerance is measured on the CPU when the cases are built: per case
and quantity ``max(100 * |oracle(order="numpy") - oracle(order="tiles")|, 1e-12)`` (``Case.tolerances()``) - the two-order deviation is
exactly the freedom the device takes.  Labels, ``n_iter``, converged, the winning restart and the selection are compared for identity
where the oracle's own margins clear the conditions (``Result.clears()``); the other cases are checked for validity.  Every figure is
printed before it is asserted."""

import warnings

import numpy as np
import pytest

import _gmm_cases as gc
import _oracle_gmm as oracle
from _baybe_shim import SearchSpace
from baybe_amd.clustering import gaussian_mixture  # noqa: F401  (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

ALL = gc.all_cases()
STEP_TOL = 1e-11
LP_TOL = 1e-10


def _torch():
    import torch

    return torch


def _device_rows(points, rows=None):
    from baybe_amd import clustering

    d = points.shape[1]
    dev = clustering.DeviceRows(points, np.zeros(d), np.ones(d))
    if rows is not None:
        dev.select(rows)
    return dev


def _rid(dev, R):
    return dev._rid(np.arange(R))


def _upload(dev, array, dtype=None):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(array)).to(dev.P.device) if dtype is None else \
        torch.from_numpy(np.ascontiguousarray(array)).to(dev.P.device, dtype)


def _spd(rng, d, cond):
    """A covariance with the given condition number."""
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    S = (Q * np.logspace(0.0, -np.log10(cond), d)) @ Q.T if d > 1 else np.ones((1, 1))
    return (S + S.T) / 2


# ---- single steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", gc.GENERIC_SHAPES, ids=lambda v: str(v))
def test_one_m_step_from_log_resp_and_from_labels(N, d):
    P = gc._normal(N, d)()
    rng = np.random.default_rng(N + d)
    R, k = 2, 5
    dev = _device_rows(P)
    torch = _torch()
    raw = rng.standard_normal((R, N, k)) * 2
    log_resp = raw - np.log(np.exp(raw).sum(axis=2, keepdims=True))
    labels = rng.integers(0, k, (R, N)).astype(np.int32)
    labels[1, : N // 3] = -1  # rows of zeros
    for source in ("log_resp", "labels"):
        params = dev.gp.gmm_params(R, k, d, dev.P.device)
        if source == "log_resp":
            dev.gp.gmm_mstep(dev.P, N, params, _rid(dev, R), 1e-6, log_resp=_upload(dev, log_resp.transpose(0, 2, 1)), normalize=True)
            resp = np.exp(log_resp)
        else:
            dev.gp.gmm_mstep(dev.P, N, params, _rid(dev, R), 1e-6, labels=_upload(dev, labels), normalize=False)
            resp = np.stack([np.where(labels[r][:, None] == np.arange(k), 1.0, 0.0) for r in range(R)])
        torch.cuda.synchronize()
        worst = 0.0
        for r in range(R):
            nk, w, means, cov = oracle.m_step(P, resp[r], 1e-6, source == "log_resp")
            got = {name: params[name][r].cpu().numpy() for name in ("nk", "w", "mu", "cov")}
            if source == "labels":
                assert np.array_equal(got["nk"], np.bincount(labels[r][labels[r] >= 0], minlength=k) + oracle.TINY)  # exact counts
            worst = max(worst, np.abs(got["nk"] - nk).max(), np.abs(got["w"] - w).max(), np.abs(got["mu"] - means).max(),
                        np.abs(got["cov"] - cov).max())
            assert np.array_equal(got["cov"], got["cov"].transpose(0, 2, 1))
        print(f"{(N, d)} {source}: worst deviation {worst:.3e}")
        assert worst <= STEP_TOL


@pytest.mark.parametrize("d", [1, 3, 15, 16, 17, 33, 64])
def test_one_precision_factor_on_covariances_of_known_condition(d):
    rng = np.random.default_rng(d)
    conds = [1.0, 1e2, 1e4, 1e6] if d > 1 else [1.0]
    cov = np.stack([_spd(rng, d, c) * s for c in conds for s in (1.0, 1e-3)])[None]  # [1, k, d, d]
    k = cov.shape[1]
    dev = _device_rows(gc._normal(4, d)())
    params = dev.gp.gmm_params(1, k, d, dev.P.device)
    params["cov"].copy_(_upload(dev, cov))
    dev.gp.gmm_precision(params, _rid(dev, 1))
    prec, logdet, flags = params["prec"][0].cpu().numpy(), params["logdet"][0].cpu().numpy(), params["flags"].cpu().numpy()
    want_prec, want_logdet, bad = oracle.precision(cov[0])
    assert not bad and flags.tolist() == [0]
    for c in range(k):
        bound = 8 * d * 2.0**-53 * np.linalg.cond(cov[0, c])
        resid = float(np.abs(prec[c].T @ cov[0, c] @ prec[c] - np.eye(d)).max())
        err = abs(logdet[c] - want_logdet[c])
        print(f"d={d} cond={np.linalg.cond(cov[0, c]):.1e}: residual {resid:.3e} logdet {err:.3e} bound {bound:.3e}")
        assert np.array_equal(prec[c], np.triu(prec[c])) and resid <= bound and err <= bound


def test_a_failed_factorisation_is_a_returned_flag():
    dev = _device_rows(gc._normal(4, 3)())
    params = dev.gp.gmm_params(3, 2, 3, dev.P.device)
    cov = np.stack([np.stack([np.eye(3), np.eye(3)]), np.stack([np.eye(3), np.zeros((3, 3))]), np.stack([-np.eye(3), np.eye(3)])])
    params["cov"].copy_(_upload(dev, cov))
    dev.gp.gmm_precision(params, _rid(dev, 3))
    assert params["flags"].cpu().numpy().tolist() == [0, 1, 1]


@pytest.mark.parametrize("N,d", gc.GENERIC_SHAPES + [(300, 3)], ids=lambda v: str(v))
def test_one_e_step_from_given_parameters(N, d):
    P = gc._normal(N, d)()
    rng = np.random.default_rng(7 * N + d)
    R, k = 2, (100 if (N, d) == (300, 3) else 4)
    torch = _torch()
    dev = _device_rows(P)
    params = dev.gp.gmm_params(R, k, d, dev.P.device)
    given = []
    for r in range(R):
        w = rng.random(k) + 0.2
        w /= w.sum()
        means = P[rng.choice(N, k, replace=False)] * 0.5
        cov = np.stack([_spd(rng, d, 1e2) * 10.0 for _ in range(k)])  # eigenvalues in [0.1, 10]: q ~ 2 d
        prec, logdet, _ = oracle.precision(cov)
        given.append((w, means, prec, logdet))
    for name, at in (("w", 0), ("mu", 1), ("prec", 2), ("logdet", 3)):
        params[name].copy_(_upload(dev, np.stack([g[at] for g in given])))
    log_resp = torch.empty((R, k, N), dtype=torch.float64, device=dev.P.device)
    labels = torch.empty((R, N), dtype=torch.int32, device=dev.P.device)
    lpn = torch.empty((R, N), dtype=torch.float64, device=dev.P.device)
    dev.gp.gmm_estep(dev.P, N, params, _rid(dev, R), log_resp, labels, 0, lpn)
    for r in range(R):
        lower, want_lr, want_labels, want_lp = oracle.e_step(P, *given[r])
        got_lr = log_resp[r].cpu().numpy().T
        got_lp = got_lr + lpn[r].cpu().numpy()[:, None]
        gap = oracle.label_gap(want_lp)
        err_lp, err_lr = float(np.abs(got_lp - want_lp).max()), float(np.abs(got_lr - want_lr).max())
        err_lb = abs(float(params["lower"][r].item()) - lower)
        print(f"{(N, d)} r={r}: lp {err_lp:.3e} log_resp {err_lr:.3e} lower bound {err_lb:.3e} label gap {gap:.3e}")
        assert gap >= 1e-6  # a condition on the fixture
        assert labels[r].cpu().numpy().tolist() == want_labels.tolist()
        assert err_lp <= LP_TOL and err_lr <= LP_TOL and err_lb <= STEP_TOL


PLANS = [  # (d, k, M) -> (components per LDS chunk, tiles per strip): 64 KB of LDS, 8 * (dpad^2 + dpad + 2 + 256) bytes a component
    ((3, 100, 300), (15, 1)), ((3, 15, 300), (15, 1)), ((3, 16, 300), (15, 1)), ((3, 2, 300), (2, 1)), ((16, 100, 300), (15, 1)),
    ((17, 12, 1000), (6, 1)), ((20, 12, 1000), (6, 1)), ((33, 5, 300), (3, 1)), ((64, 5, 400), (1, 1)),
    ((2, 3, 64 * 256), (3, 1)), ((2, 3, 64 * 256 + 1), (3, 2)), ((2, 3, 16700), (3, 2)), ((2, 3, 128 * 256 + 1), (3, 3)),
]


@pytest.mark.parametrize("shape,want", PLANS, ids=lambda v: str(v))
def test_plan_reports_the_form_at_the_chunk_and_strip_edges(shape, want):
    from baybe_amd.engine import HipGP

    gp = HipGP(0)
    assert gp.gmm_plan(*shape) == want
    gp.close()


# ---- whole fits -------------------------------------------------------------------------------------------------------------------
def _fit(case, dev):
    from baybe_amd import clustering

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the warnings' texts are host logic: tests/test_gmm_cpu.py)
        np.random.seed(case.seed)
        got = clustering._gmm_fit(dev, case.k, random_state=case.random_state, **case.kwargs())
        return got, dev.gmm_labels(), clustering._gmm_select(dev).tolist()


def _check_valid(P, case, got, labels, selection):
    """What holds for a fit whatever way its near-ties fell."""
    w, mu, cov, lower, n_iter, converged, best = got
    k = case.k
    assert np.isfinite(w).all() and np.isfinite(mu).all() and np.isfinite(cov).all() and 0 <= n_iter <= case.max_iter
    assert abs(w.sum() - 1.0) <= 1e-12
    prec, logdet, bad = oracle.precision(cov)  # the factor succeeds
    assert not bad
    lp = oracle.log_prob(P, w, mu, prec, logdet)
    assert labels.shape == (len(P),) and labels.min() >= 0 and labels.max() < k
    assert (lp[np.arange(len(P)), labels] >= lp.max(axis=1) - 1e-9).all()  # an argmax of lp, up to 1e-9
    counts = np.bincount(labels, minlength=k)
    assert len(selection) == int((counts > 0).sum())
    assert labels[selection].tolist() == np.flatnonzero(counts > 0).tolist()  # one member of every non-empty component, ascending


def _compare(case, got, labels, selection, want):
    w, mu, cov, lower, n_iter, converged, best = got
    tl = case.tolerances()
    err = {"weights": float(np.abs(w - want.weights).max()), "means": float(np.abs(mu - want.means).max()),
           "covariances": float(np.abs(cov - want.covariances).max()),
           "lower_bound": 0.0 if lower == want.lower_bound else abs(lower - want.lower_bound)}
    g = want.margins
    print(f"{case.name}: " + " ".join(f"{n} {err[n]:.3e}/{tl[n]:.1e}" for n in err) + f" n_iter {n_iter}/{want.n_iter} best {best}/{want.best} "
          f"margins label {g.label:.1e} stop {g.stop:.1e} restart {g.restart:.1e} cond {g.cond:.1e} clears {want.clears()}")
    if want.clears():
        assert labels.dtype == np.int32 and labels.tolist() == want.labels.tolist()
        assert (n_iter, converged, best, selection) == (want.n_iter, want.converged, want.best, want.selection)
        assert all(err[n] <= tl[n] for n in err)
    else:
        _check_valid(case.candidates(), case, got, labels, selection)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_device_fit_equals_the_oracle(case):
    dev = _device_rows(case.points(), case.subset())
    want = case.expected()
    if case.raises:
        with pytest.raises(ValueError, match="ill-defined empirical covariance") as err:
            _fit(case, dev)
        assert str(err.value) == str(want)
        return
    _compare(case, *_fit(case, dev), want)


def test_the_long_case():
    case = gc.LONG
    want = case.expected()
    assert want.clears(), "the long case needs another seed"
    dev = _device_rows(case.points())
    assert dev.gp.gmm_plan(2, 3, 16700) == (3, 2)  # 66 tiles in 33 strips
    _compare(case, *_fit(case, dev), want)


def test_two_runs_under_one_seed_are_identical():
    from baybe_amd import clustering

    X = gc._normal(1000, 20)()
    runs = [clustering.gaussian_mixture(X, 12, n_init=3, random_state=5, return_info=True) for _ in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][:4], runs[1][:4])) and runs[0][4:] == runs[1][4:]
    np.random.seed(5)
    again = clustering.gaussian_mixture(X, 12, n_init=3)
    assert all(np.array_equal(a, b) for a, b in zip(again, runs[0][:3]))


def test_restart_groups_give_the_same_bits(monkeypatch):
    """Three restarts as one group and as three groups of one (what ``log_resp`` beyond 1 GiB leads to)."""
    from baybe_amd import clustering

    X = gc._normal(257, 3)()
    whole = clustering.gaussian_mixture(X, 4, n_init=3, random_state=2, return_info=True)
    begin = clustering.DeviceRows.gmm_begin

    def one_per_group(self, k, reg_covar, idx=None):
        distinct, flags, _ = begin(self, k, reg_covar, idx)
        self._gm_lr, self._gm_lab = self._gm_lr[:1], self._gm_lab[:1]
        return distinct, flags, 1

    monkeypatch.setattr(clustering.DeviceRows, "gmm_begin", one_per_group)
    split = clustering.gaussian_mixture(X, 4, n_init=3, random_state=2, return_info=True)
    assert all(np.array_equal(a, b) for a, b in zip(whole[:4], split[:4])) and whole[4:] == split[4:]


def _space():
    """A search space given as a table of seeded points: a product space is all mathematical ties (rows that share coordinates), on
    which no decision can be compared."""
    import pandas as pd

    return SearchSpace.from_dataframe(pd.DataFrame(gc._normal(216, 3)(), columns=["x0", "x1", "x2"]))


def test_recommender_end_to_end_and_resident_matrix_reuse(monkeypatch):
    """``HipGaussianMixtureClusteringRecommender().recommend(8, space)`` (the reference's defaults) on seeded points returns the
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
    r = clustering.HipGaussianMixtureClusteringRecommender()
    assert r.is_available and r.model_params == {}
    np.random.seed(3)
    first = r.recommend(8, space)
    np.random.seed(3)
    want = oracle.gaussian_mixture(scaled, 8)
    print("first call:", want.margins)
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
    want = oracle.gaussian_mixture(scaled[keep], 8)
    print("second call:", want.margins)
    assert want.clears()
    assert second.index.tolist() == exp.index[np.flatnonzero(keep)[want.selection]].tolist()


def test_argument_checks_of_the_entry_points_set_the_error():
    import torch

    from baybe_amd._lib import HipError
    from baybe_amd.engine import HipGP

    gp = HipGP(0)
    P = torch.zeros((2, 256), dtype=torch.float64, device="cuda")
    wide = torch.zeros((65, 256), dtype=torch.float64, device="cuda")
    rid = torch.arange(2, dtype=torch.int32, device="cuda")
    params = gp.gmm_params(2, 3, 2, P.device)
    wide_params = gp.gmm_params(2, 3, 65, P.device)
    log_resp = torch.zeros((2, 3, 300), dtype=torch.float64, device="cuda")
    labels = torch.zeros((2, 300), dtype=torch.int32, device="cuda")
    with pytest.raises(HipError, match="bbh_gmm_plan: bad arguments .*1 <= d <= 64"):
        gp.gmm_plan(65, 3, 100)
    with pytest.raises(HipError, match="bbh_gmm_plan: bad arguments .*1 <= k <= M"):
        gp.gmm_plan(2, 101, 100)
    with pytest.raises(HipError, match="bbh_gmm_plan: bad arguments .*1 <= d <= 64"):
        gp.gmm_mstep(wide, 10, wide_params, rid, 1e-6, labels=labels)
    with pytest.raises(HipError, match="bbh_gmm_mstep: bad arguments .*ld >= M"):
        gp.gmm_mstep(P, 300, params, rid, 1e-6, labels=labels)
    with pytest.raises(HipError, match="bbh_gmm_plan: bad arguments .*1 <= k <= M"):
        gp.gmm_mstep(P, 2, params, rid, 1e-6, labels=labels)  # (the wrapper asks for the plan first)
    with pytest.raises(HipError, match="bbh_gmm_mstep: bad arguments .*log_resp or labels"):
        gp.gmm_mstep(P, 10, params, rid, 1e-6)
    with pytest.raises(HipError, match="bbh_gmm_mstep: bad arguments .*log_resp or labels"):
        gp.gmm_mstep(P, 10, params, rid, 1e-6, log_resp=log_resp, labels=labels)
    with pytest.raises(HipError, match="bbh_gmm_mstep: bad arguments .*reg_covar >= 0"):
        gp.gmm_mstep(P, 10, params, rid, -1.0, labels=labels)
    with pytest.raises(HipError, match="bbh_gmm_precision: bad arguments .*1 <= d <= 64"):
        gp.gmm_precision(wide_params, rid)
    with pytest.raises(HipError, match="bbh_gmm_estep: bad arguments .*ld >= M"):
        gp.gmm_estep(P, 300, params, rid, log_resp, labels)
    with pytest.raises(HipError, match="bbh_gmm_estep: bad arguments .*1 <= k <= M"):
        gp.gmm_estep(P, 2, params, rid, log_resp, labels)
    with pytest.raises(HipError, match="bbh_gmm_estep: bad arguments .*1 <= d <= 64"):
        gp.gmm_estep(wide, 10, wide_params, rid, log_resp, labels)
    gp.gmm_mstep(P, 10, params, rid, 1e-6, labels=labels)  # every point in component 0: the others are reg_covar I
    assert params["flags"].tolist() == [0, 0] and params["cov"][0, 1].tolist() == (1e-6 * np.eye(2)).tolist()
    gp.close()
