"""TEST INFRASTRUCTURE - k-means (Lloyd, k-means++ seeding, restarts) restated in plain numpy (no code shared with ``baybe_amd``).

Written from the k-means contract of the device path (the docstring of ``baybe_amd/clustering.py``), not from its code:

1. Positions are rows in the order given.  ``d2(x, c) = sum_k (x_k - c_k)^2`` by direct differences, k ascending (an explicit loop
   over k on numpy arrays); a label is the smallest cluster index among equal minima.
2. Generator: ``None`` -> ``np.random.mtrand._rand``, an int -> ``RandomState(int)``, an instance -> itself.  All restarts' draws
   up front: ``rs.random_sample((n_init, 1 + (k - 1) T))``, ``T = 2 + int(log k)``.  First centre: the first uniform searched, side
   right, in the normalised cumulative sum of ``1 / N``.  Further centres: ``T`` uniforms times the potential, searched in
   ``cumsum(closest)``, clipped; the candidate with the smallest new potential, first on ties.  "random": ``rs.choice(N, k,
   replace=False)`` per restart.
3. Lloyd: labels from the current centres, new centres = member sums / counts, ``shift = sum |new - old|^2``; strict stop on equal
   labels, otherwise stop on ``shift <= tol * mean(var(points, axis=0))``; labels once more after a non-strict stop; inertia = the sum
   of ``d2`` to the assigned centre; ``n_iter`` = iterations run.
4. Empty clusters: the e-th, ascending, takes the point with the e-th largest ``d2`` to its assigned old centre (ties: the smallest
   position), which leaves its old cluster's sum and count.
5. Restart choice: strictly smaller inertia AND not the same clustering up to a renaming.
6. Selection: labels from the final centres; per cluster the member with the smallest ``sqrt(d2)``, first on ties; 0 if none.

Next to the result the oracle reports how close every decision it took came to going the other way - the tests assert these as
conditions on their fixtures:

``min_margin``         the smallest gap between a point's nearest and second-nearest ``d2``, relative to the larger, over every
                       assignment of every iteration of every restart (and the final ones)
``min_seed_margin``    the same for the seeding: the distance of a searched value from the neighbouring running sums, relative to the
                       potential, and the gap between the best and the next trial potential of another candidate, relative to the larger
``min_select_margin``  the gap between the two smallest ``d2`` among a cluster's members in the selection, relative to the larger
``min_stop_gap``       the smallest ``|shift - threshold| / threshold`` over every stopping test evaluated
``min_inertia_gap``    the smallest relative inertia difference between a restart and the best so far that are not the same clustering
``ties_met``           bit-equal ties met by the first three (the stated rules decide them; they do not enter the minima above);
                       ``empties_met``: empty clusters relocated
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

import _oracle_pam

try:
    from sklearn.exceptions import ConvergenceWarning
except ImportError:  # pragma: no cover
    from baybe_amd.clustering import ConvergenceWarning

random_state = _oracle_pam.random_state
standard_scale = _oracle_pam.standard_scale


def d2_to(P: np.ndarray, c: np.ndarray) -> np.ndarray:
    """d2 of every row of ``P`` to ``c`` (``c`` [d], or [N, d] for a centre per row), in the contract's operation order."""
    acc = np.zeros(len(P))
    for k in range(P.shape[1]):
        t = P[:, k] - c[..., k]
        acc = acc + t * t
    return acc


@dataclass
class Margins:
    label: float = np.inf
    seed: float = np.inf
    select: float = np.inf
    stop: float = np.inf
    inertia: float = np.inf
    ties: int = 0
    empties: int = 0


def _rel_gap(small, large):
    """(large - small) / large elementwise, 0 where both are 0."""
    small, large = np.asarray(small, dtype=float), np.asarray(large, dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(large > 0, (large - small) / large, 0.0)


def assign(P, C, m: Margins | None = None):
    """(labels int32, d2 to the assigned centre): the first minimum over the centres in order."""
    best = np.full(len(P), np.inf)
    second = np.full(len(P), np.inf)
    lab = np.zeros(len(P), dtype=np.int32)
    for c in range(len(C)):
        v = d2_to(P, C[c])
        second = np.where(v < best, best, np.minimum(second, v))
        lab = np.where(v < best, c, lab).astype(np.int32)
        best = np.where(v < best, v, best)
    if m is not None and len(C) > 1:
        tied = second == best
        if not tied.all():
            m.label = min(m.label, float(_rel_gap(best, second)[~tied].min()))
        m.ties += int(tied.sum())
    return lab, best


def first_centres(N: int, u: np.ndarray) -> np.ndarray:
    """``rs.choice(N, p=full(N, 1 / N))`` for each uniform of ``u``."""
    cdf = np.cumsum(np.full(N, 1.0 / N))
    cdf /= cdf[-1]
    return np.minimum(np.searchsorted(cdf, u, side="right"), N - 1).astype(np.int64)


def kpp(P, k: int, first: int, u: np.ndarray, m: Margins | None = None) -> np.ndarray:
    """The centre positions of one restart: ``first``, then k - 1 centres from the uniforms ``u`` [(k - 1) T]."""
    N = len(P)
    T = 2 + int(np.log(k))
    idx = np.empty(k, dtype=np.int64)
    idx[0] = first
    closest = d2_to(P, P[first])
    pot = np.sum(closest)
    for c in range(1, k):
        rv = u[(c - 1) * T: c * T] * pot
        cum = np.cumsum(closest)
        cand = np.searchsorted(cum, rv)
        np.clip(cand, None, N - 1, out=cand)
        trial = [np.minimum(closest, d2_to(P, P[j])) for j in cand]
        pots = np.array([np.sum(t) for t in trial])
        b = int(np.argmin(pots))
        if m is not None:
            below = np.where(cand > 0, cum[np.maximum(cand - 1, 0)], -np.inf)
            near = np.minimum(np.abs(cum[cand] - rv), np.abs(rv - below))
            if pot > 0 and (near > 0).any():
                m.seed = min(m.seed, float(np.min(near[near > 0] / pot)))
            m.ties += int((near == 0).sum())
            others = (cand != cand[b]) & (pots != pots[b])
            if others.any():
                m.seed = min(m.seed, float(_rel_gap(pots[b], pots[others]).min()))
            m.ties += int(((cand != cand[b]) & (pots == pots[b])).sum())
        idx[c], closest, pot = cand[b], trial[b], pots[b]
    return idx


def update(P, labels, dmin, C, m: Margins | None = None):
    """(new centres, sums, counts before any relocation): member sums / counts, with the relocation of empty clusters."""
    k = len(C)
    sums = np.stack([P[labels == c].sum(axis=0) for c in range(k)])
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    plain = (sums.copy(), counts.copy())
    empty = np.flatnonzero(counts == 0)
    if len(empty):
        far = np.lexsort((np.arange(len(P)), -dmin))[: len(empty)]  # the largest d2 first, the smallest position among equal ones
        for e, j in zip(empty, far):
            sums[labels[j]] -= P[j]
            counts[labels[j]] -= 1
            sums[e], counts[e] = P[j], 1
        if m is not None:
            m.empties += len(empty)
    new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], sums)
    return new, plain[0], plain[1]


def lloyd(P, C0, max_iter: int, threshold: float, m: Margins | None = None):
    """One restart: (centres, labels, inertia, n_iter)."""
    C = np.array(C0, dtype=np.float64)
    old_labels = np.full(len(P), -1, dtype=np.int32)
    labels, strict, n_iter = old_labels, False, 0
    for n_iter in range(1, max_iter + 1):
        labels, dmin = assign(P, C, m)
        new, _, _ = update(P, labels, dmin, C, m)
        shift = float(np.sum((new - C) ** 2))
        C = new
        if np.array_equal(labels, old_labels):
            strict = True
            break
        if m is not None:
            m.stop = min(m.stop, abs(shift - threshold) / threshold if threshold > 0 else (np.inf if shift > 0 else 0.0))
        if shift <= threshold:
            break
        old_labels = labels
    if not strict:
        labels, _ = assign(P, C, m)
    inertia = float(np.sum(d2_to(P, C[labels])))
    return C, labels, inertia, n_iter


def same_clustering(labels, best, k: int) -> bool:
    mapping = np.full(k, -1, dtype=np.int64)
    for a, b in zip(labels, best):
        if mapping[a] == -1:
            mapping[a] = b
        elif mapping[a] != b:
            return False
    return True


def select(P, C, m: Margins | None = None) -> list:
    labels, dmin = assign(P, C, m)
    dist = np.sqrt(dmin)
    out = []
    for c in range(len(C)):
        col = np.where(labels == c, dist, np.inf)
        out.append(int(np.argmin(col)))
        members = np.sort(dmin[labels == c])
        if m is not None and len(members) > 1:
            if np.sqrt(members[0]) == np.sqrt(members[1]):
                m.ties += 1
            else:
                m.select = min(m.select, float(_rel_gap(members[0], members[1])))
    return out


@dataclass
class Result:
    centres: np.ndarray
    labels: np.ndarray
    inertia: float
    n_iter: int
    selection: list
    best: int                  # the winning restart
    seeds: np.ndarray          # [n_init, k] initial centre positions
    inertias: np.ndarray       # [n_init]
    n_iters: np.ndarray        # [n_init]
    min_margin: float = np.inf
    min_seed_margin: float = np.inf
    min_select_margin: float = np.inf
    min_stop_gap: float = np.inf
    min_inertia_gap: float = np.inf
    ties_met: int = 0
    empties_met: int = 0
    trace: list = field(default_factory=list)

    def decidable(self) -> bool:
        """Every decision either has a margin far above rounding, or is a bit-equal tie that the stated rule decides."""
        return (self.min_margin >= 1e-10 and self.min_seed_margin >= 1e-10 and self.min_select_margin >= 1e-10 and
                self.min_stop_gap >= 1e-6 and self.min_inertia_gap >= 1e-9)

    def clears(self) -> bool:
        """The conditions on a generic fixture: decidable, without ties or empty clusters."""
        return self.decidable() and self.ties_met == 0 and self.empties_met == 0


def seeds(P, k: int, n_init: int, init: str, rs) -> np.ndarray:
    N = len(P)
    if init == "random":
        return np.stack([np.asarray(rs.choice(N, k, replace=False), dtype=np.int64) for _ in range(n_init)])
    T = 2 + int(np.log(k))
    U = rs.random_sample((n_init, 1 + (k - 1) * T))
    return U, first_centres(N, U[:, 0])


def k_means(points, n_clusters, n_init="auto", max_iter=300, tol=1e-4, init="k-means++", random_state_=None) -> Result:
    P = np.asarray(points, dtype=np.float64)
    N, k = len(P), n_clusters
    rs = random_state(random_state_)
    R = (1 if init == "k-means++" else 10) if isinstance(n_init, str) else n_init
    m = Margins()
    if init == "random":
        idx = seeds(P, k, R, init, rs)
    else:
        U, first = seeds(P, k, R, init, rs)
        idx = np.stack([kpp(P, k, int(first[r]), U[r, 1:], m) for r in range(R)])
    threshold = tol * float(np.mean(np.var(P, axis=0)))
    runs = [lloyd(P, P[idx[r]], max_iter, threshold, m) for r in range(R)]
    best = 0
    for r in range(1, R):
        same = same_clustering(runs[r][1], runs[best][1], k)
        if not same:
            a, b = runs[r][2], runs[best][2]
            m.inertia = min(m.inertia, abs(a - b) / max(a, b) if max(a, b) > 0 else 0.0)
        if runs[r][2] < runs[best][2] and not same:
            best = r
    C, labels, inertia, n_iter = runs[best]
    distinct = len(np.unique(labels))
    if distinct < k:
        warnings.warn(f"Number of distinct clusters ({distinct}) found smaller than n_clusters ({k}). Possibly due to duplicate points "
                      f"in X.", ConvergenceWarning)
    return Result(C, labels, inertia, n_iter, select(P, C, m), best, idx, np.array([r[2] for r in runs]),
                  np.array([r[3] for r in runs]), m.label, m.seed, m.select, m.stop, m.inertia, m.ties, m.empties)


class OracleRows(_oracle_pam.OracleRows):
    """CPU double of the whole device surface of ``baybe_amd.clustering`` (``DeviceRows``): the k-medoids calls of
    ``_oracle_pam.OracleRows`` plus the k-means calls, answered in numpy with the arithmetic above."""

    instances = _oracle_pam.OracleRows.instances

    def mean_variance(self):
        return float(np.mean(np.var(self.P, axis=0)))

    def kmeans_seed(self, first, uniforms, k):
        return np.stack([kpp(self.P, k, int(first[r]), np.asarray(uniforms)[r]) for r in range(len(first))])

    def kmeans_begin(self, idx=None, centres=None):
        self._C = np.stack([self.P[i] for i in idx]) if centres is None else np.array(centres, dtype=np.float64)
        R = len(self._C)
        self._labels = np.full((R, self.m), -1, dtype=np.int32)
        self._inertia = np.zeros(R)
        self._sums, self._counts = np.zeros_like(self._C), np.zeros(self._C.shape[:2], dtype=np.int64)

    def kmeans_step(self, active):
        same, shift = [], []
        for r in active:
            labels, dmin = assign(self.P, self._C[r])
            new, self._sums[r], self._counts[r] = update(self.P, labels, dmin, self._C[r])
            same.append(np.array_equal(labels, self._labels[r]))
            shift.append(float(np.sum((new - self._C[r]) ** 2)))
            self._labels[r], self._C[r] = labels, new
            self._inertia[r] = np.sum(d2_to(self.P, new[labels]))
        return np.array(same, dtype=bool), np.array(shift)

    def kmeans_finish(self, nonstrict):
        for r in nonstrict:
            self._labels[r], dmin = assign(self.P, self._C[r])
            self._inertia[r] = np.sum(dmin)
        return self._inertia.copy()

    def kmeans_labels(self, r):
        return self._labels[r].copy()

    def kmeans_centres(self, r):
        return self._C[r].copy()

    def kmeans_sums(self):
        return self._sums.copy(), self._counts.copy()

    def kmeans_select(self, centres):
        return np.array(select(self.P, np.asarray(centres, dtype=np.float64)), dtype=np.int64)
