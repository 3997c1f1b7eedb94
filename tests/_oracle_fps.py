"""TEST INFRASTRUCTURE - farthest point sampling restated in exact-order arithmetic (numpy only, no code shared with ``baybe_amd``).

Written from the contract of the device path, not from its code:

1. ``d2(x, y) = sum_k (x_k - y_k) * (x_k - y_k)``: k ascending from 0.0, every subtract / multiply / add rounded to fp64 (an explicit
   loop over k on numpy arrays - numpy never contracts), squared distances compared.
2. Ranks are positions in ``np.lexsort(tuple(points.T))``; every tie rule is stated in ranks.
3. "farthest": the pair of ranks a < b with the largest d2, bit-equal maxima to the smallest a, then the smallest b; one sample
   requested: ``[a]``.
4. "random": one ``np.random.randint(0, N)``, a rank.  5. Indices: mapped to ranks.
6. Each further pick: the largest minimum d2 to the selection over unselected points; among bit-equal maxima the largest rank
   (``random_tie_break=False``) or the ``np.random.choice(count)``-th in rank order - drawn at every pick.
7. Original row indices in selection order.
8. Dead rows are never selected and never seed, and the ranks of the live rows are the restriction of the full ranking.

Besides the indices the minimum d2 at which each pick was made is returned: the pair's d2 for both points of a "farthest" start,
``inf`` for "random" / index starts (no selection existed), zeros on the all-identical path.
"""

from __future__ import annotations

import warnings

import numpy as np


def standard_scale(full: np.ndarray, rows: np.ndarray | None = None) -> np.ndarray:
    """``(rows - mean) / scale`` with the population statistics of ``full`` (numpy's ``mean`` / ``std`` over the rows of the
    row-major matrix: the summation order, and with it the last bit, follows the memory layout); a scale below 10 eps counts as 1."""
    full = np.ascontiguousarray(full, dtype=np.float64)
    mean = full.mean(axis=0)
    scale = full.std(axis=0)
    scale = np.where(scale < 10 * np.finfo(np.float64).eps, 1.0, scale)
    return ((full if rows is None else np.asarray(rows, dtype=np.float64)) - mean) / scale


def sq_dists(P: np.ndarray, y: np.ndarray) -> np.ndarray:
    """d2 of every row of ``P`` to ``y``, in the contract's operation order."""
    acc = np.zeros(len(P))
    for k in range(P.shape[1]):
        t = P[:, k] - y[k]
        acc = acc + t * t
    return acc


def farthest_pair(P: np.ndarray):
    """(d2, a, b) over positions a < b of ``P`` (already in rank order): first maximum in row-major order."""
    best, ba, bb = -np.inf, -1, -1
    for a in range(len(P) - 1):
        row = sq_dists(P[a + 1:], P[a])
        j = int(np.argmax(row))  # first maximum of the row: the smallest b
        if row[j] > best:  # strict: the smallest a stays
            best, ba, bb = row[j], a, a + 1 + j
    return best, ba, bb


def farthest_point_sampling(points, n_samples=1, initialization="farthest", random_tie_break=True, alive=None):
    """(indices, d2): original row indices in selection order and the minimum d2 each was picked at."""
    points = np.asarray(points, dtype=np.float64)
    N = len(points)
    live = np.ones(N, dtype=bool) if alive is None else np.asarray(alive, dtype=bool)
    order_full = np.lexsort(tuple(points.T))
    order = order_full[live[order_full]]  # ranks of the live rows: the restriction of the full ranking
    P = points[order]
    M = len(P)
    if len(np.unique(P, axis=0)) == 1:
        warnings.warn("All points are identical.", UserWarning)
        return np.flatnonzero(live)[:n_samples].tolist(), np.zeros(n_samples)
    if isinstance(initialization, str) and initialization == "random":
        sel, d2 = [int(np.random.randint(0, M))], [np.inf]
    elif isinstance(initialization, str) and initialization == "farthest":
        v, a, b = farthest_pair(P)
        if n_samples == 1:
            return [int(order[a])], np.array([v])
        sel, d2 = [a, b], [v, v]
    else:
        rank_of = np.empty(N, dtype=np.int64)
        rank_of[:] = -1
        rank_of[order] = np.arange(M)
        sel = [int(rank_of[i]) for i in initialization]
        assert min(sel) >= 0, "a dead row cannot seed the selection"
        d2 = [np.inf] * len(sel)
    mind = np.full(M, np.inf)
    chosen = np.zeros(M, dtype=bool)
    for s in sel:
        mind = np.minimum(mind, sq_dists(P, P[s]))
        chosen[s] = True
    while len(sel) < n_samples:
        cand = np.where(chosen, -np.inf, mind)
        top = cand.max()
        tied = np.flatnonzero(cand == top)  # rank order
        pick = int(tied[np.random.choice(len(tied))] if random_tie_break else tied[-1])
        sel.append(pick)
        d2.append(top)
        chosen[pick] = True
        mind = np.minimum(mind, sq_dists(P, P[pick]))
    return order[sel].tolist(), np.asarray(d2, dtype=np.float64)


class OraclePoints:
    """CPU double of the device surface of ``baybe_amd.sampling`` (``DevicePoints``): the same five calls, answered in numpy with the
    arithmetic above.  ``instances`` records every construction (= every upload of a point matrix)."""

    instances: list = []

    def __init__(self, values, mean, scale, device=0):
        scaled = (np.asarray(values, dtype=np.float64) - mean) / scale
        self.n, self.d = scaled.shape
        self.order = np.lexsort(tuple(scaled.T))
        self.P = scaled[self.order]
        self.calls = []
        OraclePoints.instances.append(self)

    def points(self):
        return self.P

    def _live(self, alive_ranked):
        return np.ones(self.n, dtype=bool) if alive_ranked is None else np.asarray(alive_ranked, dtype=bool)

    def all_identical(self, alive_ranked=None):
        return len(np.unique(self.P[self._live(alive_ranked)], axis=0)) == 1

    def farthest_pair(self, alive_ranked=None):
        self.calls.append(("farthest_pair", None if alive_ranked is None else int(np.sum(alive_ranked))))
        live = np.flatnonzero(self._live(alive_ranked))
        v, a, b = farthest_pair(self.P[live])
        return v, int(live[a]), int(live[b])

    def begin(self, starts, alive_ranked=None, want_count=False):
        self.calls.append(("begin", list(starts)))
        self._mind = np.where(self._live(alive_ranked), np.inf, -np.inf)
        for s in starts:
            self._take(s)
        return self._count()

    def _take(self, s):
        self._mind = np.minimum(self._mind, sq_dists(self.P, self.P[s]))
        self._mind[s] = -np.inf

    def _count(self):
        return int(np.sum(self._mind == self._mind.max()))

    def picks(self, n_picks):
        ranks, d2 = [], []
        for _ in range(n_picks):
            r, v, _ = self.pick_kth(-1, False)
            ranks.append(r)
            d2.append(v)
        return np.asarray(ranks, dtype=np.int64), np.asarray(d2)

    def pick_kth(self, k, want_count):
        top = self._mind.max()
        tied = np.flatnonzero(self._mind == top)
        r = int(tied[k])
        self._take(r)
        return r, float(top), self._count()
