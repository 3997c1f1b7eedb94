"""TEST INFRASTRUCTURE - Gaussian mixture clustering (EM, full covariances, restarts) restated in plain numpy / scipy (no code shared
with ``baybe_amd``).

Written from the Gaussian mixture contract of the device path (the docstring of ``baybe_amd/clustering.py``), not from its code:

1. Generator: ``None`` -> ``np.random.mtrand._rand``, an int -> ``RandomState(int)``, an instance -> itself.
2. Initialisation per restart, in restart order: ``"kmeans"`` - the labels of ``_oracle_kmeans.k_means(n_init=1, max_iter=300,
   tol=1e-4)``; ``"k-means++"`` - the one-hot at the k positions of its seeding; ``"random_from_data"`` - the one-hot at
   ``rs.choice(N, k, replace=False)``.
3. M-step: ``nk = sum r + 10 * 2^-52``, ``mu = sum r x / nk``, ``Sigma = sum r (x - mu)(x - mu)^T / nk + reg_covar I``, ``w = nk / N``
   (after an EM step divided by its sum, ascending).
4. Precision factor: ``Sigma = L L^T``, ``P = (L^-1)^T``, ``logdet = sum log diag P``; a factorisation that fails flags the restart
   (scikit-learn's ``ValueError``).
5. E-step: ``y = (x - mu) P``, ``lp = -0.5 (d log 2 pi + |y|^2) + logdet + log w``, ``lpn`` the log-sum-exp over the components,
   ``log_resp = lp - lpn``, label = the first maximum of ``lp``, ``lower_bound = mean lpn``.
6. Loop: E-step, M-step, ``change = lb - prev`` (``prev = -inf``), converged if ``|change| < tol``; ``max_iter = 0`` keeps the initial
   parameters.
7. Restart choice: strictly larger lower bound, or nothing kept yet; the non-convergence warning in scikit-learn's words.
8. Selection: labels from one more E-step; per non-empty component, ascending, ``t = np.random.choice(count)`` on the GLOBAL generator
   and the t-th member in position order.

``order="numpy"`` adds as numpy / BLAS / ``scipy.special.logsumexp`` do; ``order="tiles"`` adds every sum over the positions in
256-position tiles, tiles ascending, and takes the log-sum-exp as the explicit ``m + log(sum_c exp(lp - m))`` with c ascending: a
legitimate reordering, which is exactly the freedom the device takes.  The deviation between the two is the yardstick of the
whole-fit tolerance in tests/test_gmm_gpu.py.

``Margins`` reports how close the decisions came to going the other way (conditions on the fixtures, asserted on the CPU):

``label``    the smallest gap between the two largest ``lp`` of any point at prediction
``stop``     the smallest ``| |change| - tol |`` over all iterations and restarts
``restart``  the smallest gap between a restart's lower bound and the best so far
``cond``     the largest condition number of any covariance met
``flagged``  a restart's factorisation failed
``init_ok``  every decision of the k-means initialisations had a margin far above rounding (``_oracle_kmeans.Result.decidable``)
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import logsumexp

import _oracle_kmeans as okm

ConvergenceWarning = okm.ConvergenceWarning
random_state = okm.random_state
standard_scale = okm.standard_scale

TILE = 256
TINY = 10 * np.finfo(np.float64).eps
ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
               "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.")
NOT_CONVERGED = ("Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or check "
                 "for degenerate data.")


@dataclass
class Margins:
    label: float = np.inf
    stop: float = np.inf
    restart: float = np.inf
    cond: float = 0.0
    flagged: bool = False
    init_ok: bool = True


def _tiles(n):
    return [slice(a, min(a + TILE, n)) for a in range(0, n, TILE)]


def _possum(terms, n, order):
    """sum over the positions of ``terms(slice)`` (any shape): at once, or tile by tile in ascending order."""
    if order == "numpy":
        return terms(slice(0, n))
    acc = None
    for sl in _tiles(n):
        t = terms(sl)
        acc = t if acc is None else acc + t
    return acc


def m_step(P, resp, reg_covar, normalize, order="numpy", m: Margins | None = None):
    """(nk, weights, means, covariances) from the responsibilities ``resp`` [N, k]."""
    N, d = P.shape
    k = resp.shape[1]
    nk = _possum(lambda sl: resp[sl].sum(axis=0), N, order) + TINY
    means = _possum(lambda sl: resp[sl].T @ P[sl], N, order) / nk[:, None]
    cov = np.empty((k, d, d))
    for c in range(k):
        diff = P - means[c]
        cov[c] = _possum(lambda sl: (resp[sl, c] * diff[sl].T) @ diff[sl], N, order) / nk[c]
        cov[c].flat[:: d + 1] += reg_covar
        if m is not None and np.isfinite(cov[c]).all():
            m.cond = max(m.cond, float(np.linalg.cond(cov[c])))
    w = nk / N
    if normalize:
        tot = 0.0
        for c in range(k):
            tot = tot + w[c]
        w = w / tot
    return nk, w, means, cov


def precision(cov):
    """(P [k, d, d] upper triangular, logdet [k], flagged)."""
    k, d, _ = cov.shape
    prec, logdet, flagged = np.full((k, d, d), np.nan), np.full(k, np.nan), False
    for c in range(k):
        try:
            if not np.isfinite(cov[c]).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(cov[c])
        except np.linalg.LinAlgError:
            flagged = True
            continue
        prec[c] = solve_triangular(L, np.eye(d), lower=True).T
        logdet[c] = np.sum(np.log(np.diag(prec[c])))
    return prec, logdet, flagged


def log_prob(P, w, means, prec, logdet):
    """lp [N, k]."""
    N, d = P.shape
    lp = np.empty((N, len(w)))
    for c in range(len(w)):
        y = (P - means[c]) @ prec[c]
        lp[:, c] = -0.5 * (d * np.log(2 * np.pi) + np.sum(y * y, axis=1)) + logdet[c] + np.log(w[c])
    return lp


def e_step(P, w, means, prec, logdet, order="numpy"):
    """(lower bound, log_resp [N, k], labels, lp)."""
    lp = log_prob(P, w, means, prec, logdet)
    N = len(P)
    if order == "numpy":
        lpn = logsumexp(lp, axis=1)
        lower = float(np.mean(lpn))
    else:
        mx = lp.max(axis=1)
        s = np.zeros(N)
        for c in range(lp.shape[1]):
            s = s + np.exp(lp[:, c] - mx)
        lpn = mx + np.log(s)
        lower = float(_possum(lambda sl: np.sum(lpn[sl]), N, order) / N)
    return lower, lp - lpn[:, None], np.argmax(lp, axis=1).astype(np.int32), lp


def label_gap(lp) -> float:
    if lp.shape[1] < 2:
        return np.inf
    top = np.sort(lp, axis=1)[:, -2:]
    return float(np.min(top[:, 1] - top[:, 0]))


def one_hot(N, k, labels=None, idx=None):
    resp = np.zeros((N, k))
    if idx is None:
        resp[np.arange(N), labels] = 1.0
    else:
        resp[idx, np.arange(k)] = 1.0
    return resp


def initial_resp(P, k, init_params, rs, m: Margins | None = None):
    """The responsibilities one restart starts from (consumes ``rs`` as scikit-learn does)."""
    N = len(P)
    if init_params == "kmeans":
        r = okm.k_means(P, k, n_init=1, max_iter=300, tol=1e-4, random_state_=rs)
        if m is not None:
            m.init_ok = m.init_ok and r.decidable() and r.empties_met == 0
        return one_hot(N, k, labels=r.labels)
    if init_params == "k-means++":
        T = 2 + int(np.log(k))
        U = rs.random_sample((1, 1 + (k - 1) * T))
        return one_hot(N, k, idx=okm.kpp(P, k, int(okm.first_centres(N, U[:, 0])[0]), U[0, 1:]))
    if init_params == "random_from_data":
        return one_hot(N, k, idx=np.asarray(rs.choice(N, k, replace=False), dtype=np.int64))
    raise ValueError(init_params)


@dataclass
class Result:
    weights: np.ndarray
    means: np.ndarray
    covariances: np.ndarray
    labels: np.ndarray
    lower_bound: float
    n_iter: int
    converged: bool
    selection: list
    best: int
    lowers: np.ndarray
    n_iters: np.ndarray
    margins: Margins = field(default_factory=Margins)
    lp: np.ndarray = None  # of the prediction

    def clears(self) -> bool:
        """The conditions on a generic fixture."""
        g = self.margins
        return g.label >= 1e-6 and g.stop >= 1e-6 and g.restart >= 1e-9 and g.cond <= 1e4 and not g.flagged and g.init_ok


def em(P, resp, tol, reg_covar, max_iter, order="numpy", m: Margins | None = None):
    """One restart from its initial responsibilities: (params, lower bound, n_iter, converged); raises on a flagged factor."""
    _, w, means, cov = m_step(P, resp, reg_covar, False, order, m)
    prec, logdet, bad = precision(cov)
    if bad:
        if m is not None:
            m.flagged = True
        raise ValueError(ILL_DEFINED)
    lower, n_iter, converged = -np.inf, 0, False
    for n_iter in range(1, max_iter + 1):
        prev = lower
        lower, log_resp, _, _ = e_step(P, w, means, prec, logdet, order)
        _, w, means, cov = m_step(P, np.exp(log_resp), reg_covar, True, order, m)
        prec, logdet, bad = precision(cov)
        if bad:
            if m is not None:
                m.flagged = True
            raise ValueError(ILL_DEFINED)
        change = lower - prev
        if m is not None and np.isfinite(change):
            m.stop = min(m.stop, abs(abs(change) - tol))
        if abs(change) < tol:
            converged = True
            break
    return (w, means, cov, prec, logdet), lower, n_iter, converged


def select(labels, k) -> list:
    """One member of every non-empty component, ascending, drawn from the GLOBAL generator."""
    out = []
    counts = np.bincount(labels, minlength=k)
    for c in np.flatnonzero(counts > 0):
        t = np.random.choice(int(counts[c]))
        out.append(int(np.flatnonzero(labels == c)[t]))
    return out


def gaussian_mixture(points, n_components, tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params="kmeans", random_state_=None,
                     order="numpy", with_selection=True) -> Result:
    P = np.asarray(points, dtype=np.float64)
    k = n_components
    rs = random_state(random_state_)
    m = Margins()
    resps = [initial_resp(P, k, init_params, rs, m) for _ in range(n_init)]  # the draws of all restarts come first, in restart order
    runs = [em(P, resp, tol, reg_covar, max_iter, order, m) for resp in resps]
    best = -1
    for r, run in enumerate(runs):
        if best >= 0:
            m.restart = min(m.restart, abs(run[1] - runs[best][1]))
        if best < 0 or run[1] > runs[best][1]:
            best = r
    (w, means, cov, prec, logdet), lower, n_iter, converged = runs[best]
    if not converged and max_iter > 0:
        warnings.warn(NOT_CONVERGED, ConvergenceWarning)
    _, _, labels, lp = e_step(P, w, means, prec, logdet, order)
    m.label = min(m.label, label_gap(lp))
    selection = select(labels, k) if with_selection else []
    return Result(w, means, cov, labels, lower, n_iter, converged, selection, best, np.array([r[1] for r in runs]),
                  np.array([r[2] for r in runs]), m, lp)


class OracleRows(okm.OracleRows):
    """CPU double of the whole device surface of ``baybe_amd.clustering`` (``DeviceRows``): the k-medoids and k-means calls of
    ``_oracle_kmeans.OracleRows`` plus the Gaussian mixture calls, answered in numpy with the arithmetic above."""

    instances = okm.OracleRows.instances
    gmm_group = None  # restarts per group (None: all of them)

    def gmm_begin(self, k, reg_covar, idx=None):
        N = self.m
        if idx is None:
            resps = [one_hot(N, k, labels=lab) for lab in self._labels]
            distinct = np.array([len(np.unique(lab)) for lab in self._labels])
        else:
            resps = [one_hot(N, k, idx=np.asarray(i)) for i in idx]
            distinct = np.full(len(resps), k)
        self._gk, self._greg = k, reg_covar
        self._gparams, flags = [], []
        for resp in resps:
            _, w, means, cov = m_step(self.P, resp, reg_covar, False)
            prec, logdet, bad = precision(cov)
            self._gparams.append((w, means, cov, prec, logdet))
            flags.append(int(bad))
        R = len(resps)
        return distinct, np.array(flags), (R if self.gmm_group is None else min(R, self.gmm_group))

    def gmm_step(self, active, base):
        assert all(r >= base for r in active)
        lbs, flags = [], []
        for r in active:
            w, means, cov, prec, logdet = self._gparams[r]
            lower, log_resp, _, _ = e_step(self.P, w, means, prec, logdet)
            _, w, means, cov = m_step(self.P, np.exp(log_resp), self._greg, True)
            prec, logdet, bad = precision(cov)
            self._gparams[r] = (w, means, cov, prec, logdet)
            lbs.append(lower)
            flags.append(int(bad))
        return np.array(lbs), np.array(flags)

    def gmm_predict(self, r):
        w, means, _, prec, logdet = self._gparams[r]
        _, _, self._gpred, _ = e_step(self.P, w, means, prec, logdet)

    def gmm_labels(self):
        return self._gpred.copy()

    def gmm_result(self, r):
        w, means, cov, _, _ = self._gparams[r]
        return w.copy(), means.copy(), cov.copy()

    def gmm_counts(self):
        return np.bincount(self._gpred, minlength=self._gk)

    def gmm_pick(self, components, t):
        return np.array([np.flatnonzero(self._gpred == c)[i] for c, i in zip(components, t)], dtype=np.int64)
