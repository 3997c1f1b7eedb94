"""TEST INFRASTRUCTURE - k-medoids (method "alternate") restated in exact-order arithmetic (numpy only, no code shared with
``baybe_amd``).

Written from the contract of the device path (the docstring of ``baybe_amd/clustering.py``), not from its code:

1. Positions are rows in the order given.  ``d2(x, y) = sum_k (x_k - y_k) * (x_k - y_k)``: k ascending from 0.0, every subtract /
   multiply / add rounded to fp64 (an explicit loop over k on numpy arrays - numpy never contracts); ``dist = np.sqrt(d2)``;
   distances are compared and summed.
2. Every deciding sum is sequential in ascending position: the cost vector is accumulated in a loop over j (no N x N array ever
   exists), potentials are ``np.cumsum(v)[-1]``.
3. Generator: ``None`` -> ``np.random.mtrand._rand``, an int -> ``RandomState(int)``, an instance -> itself.
4. "k-medoids++": ``T = 2 + int(log k)``, ``c0 = rs.randint(N)``, ``closest = dist(c0, .)^2``, per further centre
   ``rs.random_sample(T) * pot`` -> ``searchsorted(cumsum(closest))``, trials in order, the first or a strictly smaller potential
   wins.  "random": ``rs.choice(N, k, replace=False)``.
5. Iteration: labels = first minimum over clusters; per cluster (empty: warn, skip) costs over the members, the first minimum, adopted
   iff strictly below the medoid's cost (the first member's if the medoid is not a member); stop when nothing changed; warn on the
   last permitted iteration otherwise.
6. Result: medoids, final labels, ``np.sum`` of the distances to the assigned medoids, the index of the last iteration run.

``ties_met`` counts how often a bit-equal tie DECIDED something: a label whose minimum is shared by two clusters, a cost minimum
shared by two members, ``min_cost == curr_cost`` at a row other than the medoid, a trial potential equal to the best so far.
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

from sklearn.exceptions import ConvergenceWarning


def dists(P: np.ndarray, y: np.ndarray) -> np.ndarray:
    """dist of every row of ``P`` to ``y``, in the contract's operation order."""
    acc = np.zeros(len(P))
    for k in range(P.shape[1]):
        t = P[:, k] - y[k]
        acc = acc + t * t
    return np.sqrt(acc)


def seqsum(v: np.ndarray) -> float:
    return np.cumsum(v)[-1]


def random_state(seed):
    if seed is None:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(seed)
    return seed


@dataclass
class Result:
    medoids: list
    labels: np.ndarray
    inertia: float
    n_iter: int
    ties_met: int
    first_costs: np.ndarray = None  # cost of every position in the first iteration (None: max_iter = 0)
    dist: np.ndarray = None         # distance of every position to its final medoid
    trace: list = field(default_factory=list)


def assign(P, medoids):
    """(labels, dist, ties): the first minimum over the clusters in order."""
    best = np.full(len(P), np.inf)
    lab = np.zeros(len(P), dtype=np.int32)
    tied = np.zeros(len(P), dtype=bool)
    for c, m in enumerate(medoids):
        v = dists(P, P[m])
        tied = np.where(v < best, False, tied | (v == best))
        lab = np.where(v < best, c, lab).astype(np.int32)
        best = np.where(v < best, v, best)
    return lab, best, int(tied.sum())


def cluster_costs(P, members):
    """cost[a] = sum over the members b, ascending, of dist(members[a], members[b])."""
    Q = P[members]
    cost = np.zeros(len(members))
    for j in range(len(members)):
        cost = cost + dists(Q, Q[j])
    return cost


def kpp_init(P, k, rs):
    n = len(P)
    ties = 0
    centers = np.empty(k, dtype=np.int64)
    T = 2 + int(np.log(k))
    centers[0] = rs.randint(n)
    row = dists(P, P[centers[0]])
    closest = row * row
    pot = seqsum(closest)
    for c in range(1, k):
        rv = rs.random_sample(T) * pot
        cand = np.searchsorted(np.cumsum(closest), rv)
        best = best_pot = best_closest = None
        for t in range(T):
            r = dists(P, P[cand[t]])
            new = np.minimum(closest, r * r)
            new_pot = seqsum(new)
            if best is not None and new_pot == best_pot and cand[t] != best:
                ties += 1
            if best is None or new_pot < best_pot:
                best, best_pot, best_closest = cand[t], new_pot, new
        centers[c], pot, closest = best, best_pot, best_closest
    return centers, ties


def k_medoids(points, n_clusters, max_iter=100, init="k-medoids++", random_state_=None) -> Result:
    P = np.asarray(points, dtype=np.float64)
    n, k = len(P), n_clusters
    rs = random_state(random_state_)
    ties = 0
    if init == "random":
        medoids = np.asarray(rs.choice(n, k, replace=False), dtype=np.int64)
    else:
        medoids, ties = kpp_init(P, k, rs)
    first_costs = None
    n_iter = 0
    for n_iter in range(max_iter):
        old = medoids.copy()
        lab, _, t = assign(P, medoids)
        ties += t
        costs_all = np.full(n, np.nan)
        for c in range(k):
            members = np.flatnonzero(lab == c)
            if len(members) == 0:
                warnings.warn("Cluster {k} is empty! self.labels_[self.medoid_indices_[{k}]] may not be labeled with its "
                              "corresponding cluster ({k}).".format(k=c))
                continue
            cost = cluster_costs(P, members)
            costs_all[members] = cost
            a = int(np.argmin(cost))
            ties += int(np.sum(cost == cost[a]) > 1)
            at = np.flatnonzero(members == medoids[c])
            cur = int(at[0]) if len(at) else 0
            if cost[a] == cost[cur] and a != cur:
                ties += 1
            if cost[a] < cost[cur]:
                medoids[c] = members[a]
        if first_costs is None:
            first_costs = costs_all
        if np.all(old == medoids):
            break
        elif n_iter == max_iter - 1:
            warnings.warn("Maximum number of iteration reached before convergence. Consider increasing max_iter to improve the fit.",
                          ConvergenceWarning)
    lab, dist, t = assign(P, medoids)
    ties += t
    return Result([int(m) for m in medoids], lab, float(np.sum(dist)), n_iter, ties, first_costs, dist)


def standard_scale(full: np.ndarray) -> np.ndarray:
    full = np.ascontiguousarray(full, dtype=np.float64)
    mean = full.mean(axis=0)
    scale = full.std(axis=0)
    scale = np.where(scale < 10 * np.finfo(np.float64).eps, 1.0, scale)
    return (full - mean) / scale


class OracleRows:
    """CPU double of the device surface of ``baybe_amd.clustering`` (``DeviceRows``): the same calls, answered in numpy with the
    arithmetic above.  ``instances`` records every construction (= every upload of a matrix), ``selects`` every candidate set."""

    instances: list = []

    def __init__(self, values, mean, scale, device=0):
        self.scaled = (np.asarray(values, dtype=np.float64) - mean) / scale
        self.n, self.d = self.scaled.shape
        self.selects = []
        OracleRows.instances.append(self)
        self.select(None)

    def select(self, rows=None):
        self.selects.append(None if rows is None else np.asarray(rows).copy())
        self.P = self.scaled if rows is None else self.scaled[np.asarray(rows)]
        self.m = len(self.P)

    def dist_rows(self, rows):
        return np.stack([dists(self.P, self.P[r]) for r in rows])

    def assign(self, medoids):
        lab, dist, _ = assign(self.P, medoids)
        return lab, dist

    def step(self, medoids):
        medoids = np.asarray(medoids, dtype=np.int64).copy()
        lab, _, _ = assign(self.P, medoids)
        self._costs = np.full(self.m, np.nan)
        empty, changed = [], False
        for c in range(len(medoids)):
            members = np.flatnonzero(lab == c)
            if len(members) == 0:
                empty.append(c)
                continue
            cost = cluster_costs(self.P, members)
            self._costs[members] = cost
            a = int(np.argmin(cost))
            at = np.flatnonzero(members == medoids[c])
            if cost[a] < cost[int(at[0]) if len(at) else 0]:
                changed = changed or members[a] != medoids[c]
                medoids[c] = members[a]
        return medoids, empty, bool(changed)

    def costs(self):
        return self._costs
