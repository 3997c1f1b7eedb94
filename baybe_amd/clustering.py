"""k-medoids, k-means and Gaussian mixture clustering on the device, and the initial recommenders built on them (k-medoids first;
the k-means and Gaussian mixture contracts follow it).

``k_medoids`` mirrors the reference's own ``KMedoids`` with ``method="alternate"``
(``baybe/utils/clustering_algorithms/third_party/kmedoids.py``: same validation and error texts, same warnings, the same draws from the
same generator) and ``HipPAMRecommenderImpl._recommend_discrete`` mirrors ``SKLearnClusteringRecommender._recommend_discrete`` with
``PAMClusteringRecommender``'s selection (``baybe/recommenders/pure/nonpredictive/clustering.py:100-132, 174-193``), without the N x N
distance matrix the reference builds on the host (``kmedoids.py:231``: 80 GB at 1e5 candidates).  The kernels are in
``csrc/bbh_pam.hip``.

The contract (``tests/_oracle_pam.py`` restates it in numpy, from these words):

Positions are the rows of the point matrix in the order given - the reference does not sort here, so there are no ranks - and every
tie goes to the first in position / cluster order, which is what numpy's ``argmin`` gives the reference on equal values.

Arithmetic.  ``d2(x, y) = sum_k (x_k - y_k) * (x_k - y_k)``, k ascending from 0.0, nothing contracted; ``dist = sqrt(d2)``, IEEE,
correctly rounded (bit-equal to ``np.sqrt``); distances, not squares, are compared and summed; every sum that decides something is
sequential in ascending position (``np.cumsum(v)[-1]``).

Generator.  ``random_state=None``: ``np.random.mtrand._rand`` (what ``check_random_state(None)`` returns); an int: ``RandomState(int)``;
an instance: itself.

``init="k-medoids++"`` (``kmedoids.py:438-511``).  ``T = 2 + int(np.log(k))``; ``c0 = rs.randint(N)``; ``closest = dist(c0, .) *
dist(c0, .)`` (the reference squares the stored distance); ``pot = seqsum(closest)``; for each further centre ``rv =
rs.random_sample(T) * pot``, ``cand = np.searchsorted(np.cumsum(closest), rv)``, and the trials run in order: ``new = minimum(closest,
dist(cand_t, .)^2)``, kept if it is the first trial or ``seqsum(new) < best_pot`` strictly.  ``init="random"``: ``rs.choice(N, k,
replace=False)``.

Iteration (``kmedoids.py:254-292``), at most ``max_iter`` times.  ``label[j]``: the smallest cluster index among bit-equal minima of
``dist(medoid_c, j)``.  For every cluster, from the labels of this iteration: an empty cluster warns in the reference's words and is
skipped; ``cost[i] = sum over the members j, ascending, of dist(i, j)`` for each member i; the new medoid is the smallest position
among bit-equal minima, adopted only if ``min_cost < curr_cost`` strictly, where ``curr_cost`` is the medoid's cost - or the first
member's if the medoid is not a member of its own cluster (duplicate rows; ``np.argmax(cluster_k_idxs == medoid)`` yields 0).  Stop
when no medoid changed; a last permitted iteration that still changed one warns with the reference's ``ConvergenceWarning`` text.

Result.  Medoid positions in cluster order; final labels, assigned once more from the final medoids; ``inertia = np.sum`` of the
distance-to-assigned-medoid vector on the host; ``n_iter``, the reference's ``n_iter_``: the index of the last iteration run (0 for
``max_iter = 0``).

On points in generic position this reproduces the reference's ``medoid_indices_``; where costs are mathematically tied (grids,
duplicates, two-member clusters) the reference's choice follows the rounding of sklearn's ``|x|^2 + |y|^2 - 2 x.y`` matrix and the rule
above decides instead.


k-means.  ``k_means`` is the counterpart of ``sklearn.cluster.KMeans(n_clusters, n_init=..., max_iter=..., tol=..., init=...,
random_state=...).fit`` as the reference's ``KMeansClusteringRecommender`` drives it (``nonpredictive/clustering.py:196-252``, defaults
``{"max_iter": 1000, "n_init": 50}``), and ``HipKMeansRecommenderImpl._recommend_discrete`` adds that class's selection.  All
``n_init`` restarts are one device workload (``csrc/bbh_kmeans.hip``): a pass reads each point once per restart TILE, not once per
restart.  The contract is this project's own arithmetic, not bit-parity with scikit-learn's BLAS form
(``tests/_oracle_kmeans.py`` restates it in numpy, from these words; device results are held to it within a tolerance, and every
decision that rests on a comparison is tested where the oracle's own margin is far larger):

Positions and arithmetic.  Points are the rows in the order given.  ``d2(x, c) = sum_k (x_k - c_k)^2`` by direct differences in
fp64, k ascending; there is no ``|x|^2 + |c|^2 - 2 x.c`` form and no mean-centring (direct differences do not need it).  A label is
the smallest cluster index among equal minima of ``d2``.

Generator.  The one ``_random_state`` returns.  A restart's draws are ``1 + (k - 1) T`` uniforms with ``T = 2 + int(log k)``,
whatever the data, so the draws of all ``n_init`` restarts are taken up front, in restart order, as scikit-learn would consume them:
``rs.random_sample((n_init, 1 + (k - 1) T))``.  First centre: ``choice(N, p=uniform)``, i.e. the row's first uniform searched, side
right, in ``cumsum(full(N, 1 / N))`` divided by its last entry.  Each further centre: the next ``T`` uniforms times ``pot`` (the sum
of ``closest``, the ``d2`` of every point to its nearest centre so far) are searched (side left) in the running sum of ``closest``,
clipped to ``N - 1``; the candidate with the smallest new potential ``sum(minimum(closest, d2(., x_cand)))`` is taken, the first on
ties.  ``init="random"``: ``rs.choice(N, k, replace=False)`` per restart, in restart order.

Lloyd, at most ``max_iter`` times per restart.  Each iteration computes labels from the current centres, then new centres as member
sums divided by counts (a cluster whose count is zero after a relocation keeps its sum), and ``shift = sum over centres of
|new - old|^2``.  Stop if the labels equal the previous iteration's labels (strict); otherwise stop if ``shift <= tol *
mean(var(points, axis=0))``.  After a non-strict stop - the iteration limit included - labels are assigned once more from the final
centres.  ``inertia`` is the sum of ``d2`` to the assigned (final) centre; ``n_iter`` is the number of iterations run.

Empty clusters.  The e-th empty cluster, in ascending index, takes the point with the e-th largest ``d2`` to its assigned old
centre (ties: the smallest position); that point is removed from its old cluster's sum and count, its label stays.  This is
scikit-learn's relocation, made deterministic.

Restart choice.  The first restart is the best so far; a later one replaces it only if its inertia is strictly smaller AND its
labels are not the same clustering up to a renaming of the clusters (every label of the later restart meets a single label of the
best) - scikit-learn's rule.  If the winner has fewer distinct labels than clusters, scikit-learn's ``ConvergenceWarning`` is raised
in its words.

Selection (``KMeansClusteringRecommender._make_selection_custom``).  Labels are assigned from the final centres of the winner; per
cluster, in cluster order, the position with the smallest ``sqrt(d2)`` among its own members is taken, the first on ties.  A
cluster without members yields position 0, as ``argmin`` of an all-infinite column does in the reference.

``max_iter = 0`` is a scikit-learn validation error in ``k_means`` and the recommender; the contract itself (``_kmeans_fit``, the
oracle) covers it: no iteration, labels from the initial centres, ``n_iter = 0``.


Gaussian mixture.  ``gaussian_mixture`` is the counterpart of ``sklearn.mixture.GaussianMixture(n_components, ...).fit`` as the
reference's ``GaussianMixtureClusteringRecommender`` drives it (``nonpredictive/clustering.py:255-304``, ``model_params = {}``), and
``HipGMMRecommenderImpl._recommend_discrete`` adds the selection that class really makes: ``_make_selection_default``
(``clustering.py:55-76``) - the class does not set ``_use_custom_selector``, so its density selector is never run.  The kernels are
in ``csrc/bbh_gmm.hip``.  As with k-means this is the project's own arithmetic, held to the oracle within a tolerance
(``tests/_oracle_gmm.py`` restates it in numpy, from these words), not bit-parity with BLAS.

Arguments and defaults.  ``n_components``, ``covariance_type="full"``, ``tol=1e-3``, ``reg_covar=1e-6``, ``max_iter=100``,
``n_init=1``, ``init_params="kmeans"``, ``random_state=None``.  Generator: the one ``_random_state`` returns.

Initialisation, per restart in restart order; a label of -1 marks a row of zeros.  ``"kmeans"``: the labels of the k-means contract
above with ``n_init=1, max_iter=300, tol=1e-4, init="k-means++"``; a restart consumes ``1 + (k - 1) T`` uniforms whatever the data, so
the draws of all R initialisations are taken up front as ``rs.random_sample((R, 1 + (k - 1) T))`` and run side by side as R restarts
of one k-means pass - every restart's labels are used, none is chosen; scikit-learn's "distinct clusters" warning applies per
restart.  ``"k-means++"``: the k positions of the k-means++ seeding of a restart, one-hot at those k rows only.
``"random_from_data"``: ``rs.choice(N, k, replace=False)``, one-hot at those rows.  ``"random"`` is refused (it needs an [N, k]
upload).

M-step, from labels (one-hot) or from ``resp = exp(log_resp)``.  ``nk_c = sum_j r_jc + 10 * 2^-52``; ``mu_c = (sum_j r_jc x_j) /
nk_c``; ``Sigma_c = (sum_j r_jc (x_j - mu_c)(x_j - mu_c)^T) / nk_c``, then ``+ reg_covar`` on the diagonal; ``w_c = nk_c / N``, and
after an EM step ``w`` is also divided by ``sum_c w_c``, added in ascending c.

Precision factor.  ``Sigma_c = L L^T`` (lower Cholesky); ``P_c = (L^-1)^T`` (upper triangular); ``logdet_c = sum_i log P_c[i, i]``
(ascending i; the device carries the rounding error of every addition along, since d terms of one sign lose ulps of a large total).
A pivot that is not finite and positive flags the restart, and the host raises scikit-learn's ``ValueError`` ("Fitting the mixture
model failed because some components have ill-defined empirical covariance ...").

E-step.  ``y = (x_j - mu_c) @ P_c`` and ``q = sum_i y_i^2``; ``lp_jc = -0.5 * (d * log(2 pi) + q) + logdet_c + log(w_c)``;
``lpn_j = m + log(sum_c exp(lp_jc - m))`` with ``m = max_c lp_jc`` and c ascending; ``log_resp_jc = lp_jc - lpn_j``; ``label_j`` is
the smallest c among equal maxima of ``lp_jc`` (this is ``predict``); ``lower_bound = (sum_j lpn_j) / N``.

Loop, per restart, for ``n_iter = 1 .. max_iter``: E-step; M-step and precision factor; ``change = lb - prev`` with ``prev = -inf``
at first; stop, converged, if ``|change| < tol``.  ``max_iter = 0`` keeps the initial parameters, ``n_iter = 0``, a lower bound of
``-inf``, and gives no warning.

Restart choice.  A restart replaces the best so far if its lower bound is strictly larger, or if nothing was kept yet.  If the
winner did not converge and ``max_iter > 0``, scikit-learn's ``ConvergenceWarning`` is raised in its words ("Best performing
initialization did not converge. ...").

Prediction and selection.  One more E-step from the winner's parameters gives the labels; the member counts per component give the
non-empty components, ascending; for each of them ``t = np.random.choice(count_c)`` - the GLOBAL generator, after the fit, consumed
exactly as the reference's ``np.random.choice(members)`` consumes it - and the pick is the t-th member in position order.  A
component without members yields no row: fewer than ``batch_size`` rows can come back.

Fixed-shape sums.  Every sum has a fixed shape: positions ascending inside a strip of 256-position tiles, strips ascending, or the
MFMA's own order, which the hardware fixes.  There are no floating-point atomics; two runs under one seed give the same bits.

Refused before anything goes to the device: first scikit-learn's own texts for bad values of ``n_components``, ``tol``,
``reg_covar``, ``max_iter``, ``n_init``, ``covariance_type`` and ``init_params``, for fewer than 2 samples and for ``n_samples <
n_components``; then what the HIP path leaves out: a ``covariance_type`` other than ``"full"``, ``init_params="random"``,
``weights_init`` / ``means_init`` / ``precisions_init``, ``warm_start``, more than 64 columns, and more than 65535 components (a
grid dimension of the kernels).  The limit of 64 columns: full
covariances cost ``k d^2`` doubles and their factorisation is one workgroup's work (64 x 64 doubles are 32 KB of LDS); wider comp
reps go to k-means, whose limit stays 768.
"""

from __future__ import annotations

import warnings
from typing import ClassVar

import attrs
import numpy as np
import pandas as pd
from attrs import field
from attrs.validators import instance_of

from baybe_amd.sampling import HipFPSRecommenderImpl, _StandAloneFPS, standard_scaling

try:  # the reference warns with sklearn's class; a filter on it must catch ours too
    from sklearn.exceptions import ConvergenceWarning
except ImportError:  # pragma: no cover

    class ConvergenceWarning(UserWarning):
        """Stand-in for ``sklearn.exceptions.ConvergenceWarning`` where sklearn is not installed."""


_INIT_METHODS = ["random", "heuristic", "k-medoids++", "build"]
_MAX_D = 768
_MAX_ROWS = 2**31 - 256


class DeviceRows:
    """A point matrix resident on the device (``X [n, d]`` as uploaded, with the scaling that turns it into points) and the dense
    matrix ``P [d, ldp]`` of the rows currently selected, on a model-less ``HipGP`` handle.  This is the whole device surface of the
    module: the tests double it on the CPU."""

    def __init__(self, values: np.ndarray, mean: np.ndarray, scale: np.ndarray, device: int = 0):
        from baybe_amd.engine import HipGP

        self.gp = HipGP(device)
        self.n, self.d = values.shape
        self.mean, self.scale = mean, scale
        self.X = self._upload(values)
        self.select(None)

    def _upload(self, values: np.ndarray):
        import torch

        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(self.gp._dev())

    def select(self, rows=None):
        """The points of the calls that follow: the rows ``rows`` of the matrix, in that order (``None``: all of them)."""
        import torch

        order = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.X.device)
        self.m = self.n if rows is None else len(rows)
        self.P = self.gp.fps_prepare(self.X, self.mean, self.scale, order)
        self._cost = self._perm = None

    def _index(self, idx):
        import torch

        return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.P.device)

    def dist_rows(self, rows) -> np.ndarray:
        """[T, m]: the distances from the positions ``rows`` to every position."""
        return self.gp.pam_dist_rows(self.P, self.m, self._index(rows)).cpu().numpy()

    def assign(self, medoids):
        """(labels int32 [m], dist [m]) on the host."""
        labels, dist = self.gp.pam_assign(self.P, self.m, self._index(medoids))
        return labels.cpu().numpy(), dist.cpu().numpy()

    def step(self, medoids):
        """One iteration: (medoids after the update, indices of the empty clusters, whether a medoid changed).  Labels, the stable
        grouping, the cost pass and the update are enqueued back to back; reading the medoids and flags is the one synchronisation."""
        import torch

        k, m = len(medoids), self.m
        med = self._index(medoids)
        labels, _ = self.gp.pam_assign(self.P, m, med)
        grouped, perm = torch.sort(labels, stable=True)  # grouped by label, position order kept inside a cluster
        # the clusters' column ranges [k + 1], without a read-back (bincount would take one for its bin count)
        starts = torch.searchsorted(grouped, torch.arange(k + 1, dtype=torch.int32, device=labels.device))
        zero = torch.zeros(1, dtype=torch.int64, device=labels.device)
        tile_starts = torch.cat([zero, torch.cumsum((starts[1:] - starts[:-1] + 255) // 256, 0)])
        Ps = self.P.index_select(1, perm)
        cost = self.gp.pam_cost(Ps, m, starts, tile_starts, k)
        flags = self.gp.pam_update(cost, perm, m, starts, med)
        self._cost, self._perm = cost, perm
        out = torch.cat([med, flags.to(torch.int64)]).cpu().numpy()
        f = out[k:]
        return out[:k].copy(), np.flatnonzero(f == 1).tolist(), bool((f == 2).any())

    def costs(self) -> np.ndarray:
        """The in-cluster cost of every position as the last ``step`` computed it (before its update)."""
        import torch

        cost = torch.empty_like(self._cost)
        cost[self._perm] = self._cost
        return cost.cpu().numpy()

    # ---- k-means: R restarts side by side.  Centres [R, k, d], labels [R, m] and d2 [R, m] stay on the device. ----
    def mean_variance(self) -> float:
        """``mean(var(points, axis=0))``: the scale of the stopping tolerance."""
        return float(self.P[:, : self.m].var(dim=1, unbiased=False).mean().item())

    def kmeans_seed(self, first, uniforms, k: int) -> np.ndarray:
        """k-means++ for all restarts at once: the centre positions [R, k], column 0 = ``first``; ``uniforms`` [R, (k - 1) T].
        ``closest``, the trial potentials, the running sum and the search stay on the device."""
        import torch

        R = len(first)
        idx = torch.zeros((R, k), dtype=torch.int64, device=self.P.device)
        idx[:, 0] = self._index(first)
        U = None if k == 1 else torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64)).to(self.P.device)
        self._km_d2 = torch.empty((R, self.m), dtype=torch.float64, device=self.P.device)  # closest now, d2 of the passes later
        self.gp.kmeans_seed(self.P, self.m, idx, U, 2 + int(np.log(k)), closest=self._km_d2)
        return idx.cpu().numpy()

    def kmeans_begin(self, idx=None, centres=None):
        """Starts R restarts from the points at the positions ``idx`` [R, k] (or from ``centres`` [R, k, d]); no labels yet."""
        import torch

        if centres is None:
            R, k = idx.shape
            self._km_C = self.P.index_select(1, self._index(np.reshape(idx, -1))).T.contiguous().reshape(R, k, self.d)
        else:
            self._km_C = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float64)).to(self.P.device)
            R = self._km_C.shape[0]
        self._km_labels = torch.full((R, self.m), -1, dtype=torch.int32, device=self.P.device)
        if getattr(self, "_km_d2", None) is None or tuple(self._km_d2.shape) != (R, self.m):
            self._km_d2 = torch.empty((R, self.m), dtype=torch.float64, device=self.P.device)
        self._km_out = None
        self._km_relocated = np.zeros(R, dtype=bool)

    def _rid(self, restarts):
        import torch

        return torch.from_numpy(np.ascontiguousarray(restarts, dtype=np.int32)).to(self.P.device)

    def kmeans_step(self, active):
        """One Lloyd iteration of the restarts ``active``: (labels unchanged [len(active)] bool, shift [len(active)]).  The pass
        and its finish are enqueued per restart tile; reading the shifts and flags is the one synchronisation.  A restart that met
        an empty cluster takes the host path for this iteration (``_relocate``)."""
        import torch

        rid = self._rid(active)
        out = self._km_out = self.gp.kmeans_pass(self.P, self.m, self._km_C, rid, self._km_labels, self._km_d2, self._km_out)
        rid = rid.long()
        host = torch.cat([out["shift"][rid], out["flags"][rid].double()]).cpu().numpy()
        shift, flags = host[: len(active)].copy(), host[len(active):].astype(np.int64)
        self._km_relocated[np.asarray(active)] = False
        for a in np.flatnonzero(flags & 2):
            shift[a] = self._relocate(int(active[a]))
        self._km_C[rid] = out["new"][rid]
        return (flags & 1).astype(bool), shift

    def _relocate(self, r: int) -> float:
        """The empty clusters of restart ``r`` after its pass, on the host: the e-th of them takes the point with the e-th largest
        d2 (ties: the smallest position).  Writes the new centres, returns the shift."""
        import torch

        out = self._km_out
        labels, d2 = self._km_labels[r].cpu().numpy(), self._km_d2[r].cpu().numpy()
        sums, counts = out["sums"][r].cpu().numpy(), out["counts"][r].cpu().numpy().astype(np.int64)
        old = self._km_C[r].cpu().numpy()
        empty = np.flatnonzero(counts == 0)
        far = np.lexsort((np.arange(self.m), -d2))[: len(empty)]
        rows = self.P.index_select(1, self._index(far)).T.cpu().numpy()
        for e, j, x in zip(empty, far, rows):
            sums[labels[j]] -= x
            counts[labels[j]] -= 1
            sums[e], counts[e] = x, 1
        new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], sums)
        out["new"][r] = torch.from_numpy(new).to(self.P.device)
        self._km_relocated[r] = True
        return float(np.sum((new - old) ** 2))

    def kmeans_finish(self, nonstrict) -> np.ndarray:
        """Assigns the labels of the restarts ``nonstrict`` once more from their final centres; the inertia of every restart [R]."""
        if len(nonstrict):
            self._km_out = self.gp.kmeans_pass(self.P, self.m, self._km_C, self._rid(nonstrict), self._km_labels, self._km_d2, self._km_out,
                                               want_sums=False)
            self._km_relocated[np.asarray(nonstrict, dtype=np.int64)] = False
        inertia = self._km_out["inertia"].cpu().numpy().copy()
        for r in np.flatnonzero(self._km_relocated):  # a strict stop in an iteration that relocated: the centres moved after the pass
            pts, C, lab = self.P[:, : self.m].T.cpu().numpy(), self._km_C[r].cpu().numpy(), self._km_labels[r].cpu().numpy()
            acc = np.zeros(self.m)
            for k in range(self.d):
                t = pts[:, k] - C[lab, k]
                acc = acc + t * t
            inertia[r] = np.sum(acc)
        return inertia

    def kmeans_labels(self, r: int) -> np.ndarray:
        return self._km_labels[r].cpu().numpy()

    def kmeans_centres(self, r: int) -> np.ndarray:
        return self._km_C[r].cpu().numpy()

    def kmeans_sums(self):
        """(sums [R, k, d], counts [R, k]) of the members as the last ``kmeans_step`` added them (before any relocation)."""
        return self._km_out["sums"].cpu().numpy(), self._km_out["counts"].cpu().numpy()

    def kmeans_select(self, centres) -> np.ndarray:
        """The reference's selection from ``centres`` [k, d]: per cluster the member nearest to its centre (a masked argmin on the
        device, no [N, k] array anywhere); position 0 for a cluster without members."""
        import torch

        dev = self.P.device
        C = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float64)[None]).to(dev)
        labels = torch.full((1, self.m), -1, dtype=torch.int32, device=dev)
        d2 = torch.empty((1, self.m), dtype=torch.float64, device=dev)
        self.gp.kmeans_pass(self.P, self.m, C, torch.zeros(1, dtype=torch.int32, device=dev), labels, d2, None, want_sums=False)
        return self.gp.kmeans_select(labels[0], d2[0], C.shape[1]).cpu().numpy()

    # ---- Gaussian mixture: R restarts side by side.  Parameters [R, ...], log_resp [G, k, m] and labels [G, m] stay on the device. ----
    def gmm_begin(self, k: int, reg_covar: float, idx=None):
        """Starts R restarts with an M-step from labels - the labels the last k-means run left (``idx`` None), or the one-hot at the
        positions ``idx`` [R, k] - and their precision factors: (components with members [R], failure flags [R], G = the restarts
        that share a group, so that ``log_resp`` [G, k, m] stays under 1 GiB)."""
        import torch

        dev = self.P.device
        if idx is None:
            labels = self._km_labels
        else:
            pos = self._index(idx)
            labels = torch.full((pos.shape[0], self.m), -1, dtype=torch.int32, device=dev)
            labels.scatter_(1, pos, torch.arange(k, dtype=torch.int32, device=dev).expand(pos.shape[0], k).contiguous())
        R = int(labels.shape[0])
        self._gm = self.gp.gmm_params(R, k, self.d, dev)
        self._gm_reg = float(reg_covar)
        G = max(1, min(R, 2**30 // (8 * k * self.m)))
        self._gm_lr = torch.empty((G, k, self.m), dtype=torch.float64, device=dev)
        self._gm_lab = torch.empty((G, self.m), dtype=torch.int32, device=dev)
        self.gp.gmm_mstep(self.P, self.m, self._gm, self._rid(np.arange(R)), reg_covar, labels=labels, normalize=False)
        flat = labels.long() + torch.arange(R, device=dev)[:, None] * k
        members = torch.bincount(flat[labels >= 0], minlength=R * k).view(R, k)
        host = torch.cat([(members > 0).sum(1), self._gm["flags"].long()]).cpu().numpy()
        return host[:R].copy(), host[R:].copy(), G

    def gmm_step(self, active, base: int):
        """One EM iteration of the restarts ``active`` (all inside the group that begins at restart ``base``): (lower bound of the
        E-step [len(active)], failure flags after the M-step [len(active)]).  E-step, M-step and precision factors are enqueued back
        to back; reading the bounds and flags is the one synchronisation."""
        import torch

        rid = self._rid(active)
        self.gp.gmm_estep(self.P, self.m, self._gm, rid, self._gm_lr, self._gm_lab, base)
        self.gp.gmm_mstep(self.P, self.m, self._gm, rid, self._gm_reg, log_resp=self._gm_lr, base=base, normalize=True)
        rid = rid.long()
        host = torch.cat([self._gm["lower"][rid], self._gm["flags"][rid].double()]).cpu().numpy()
        return host[: len(active)].copy(), host[len(active):].astype(np.int64)

    def gmm_predict(self, r: int):
        """One more E-step from the parameters of restart ``r``: its labels stay on the device (``gmm_labels`` reads them)."""
        self.gp.gmm_estep(self.P, self.m, self._gm, self._rid([r]), self._gm_lr, self._gm_lab, r)
        self._gm_pred = self._gm_lab[0]

    def gmm_labels(self) -> np.ndarray:
        return self._gm_pred.cpu().numpy()

    def gmm_result(self, r: int):
        """(weights [k], means [k, d], covariances [k, d, d]) of restart ``r``."""
        return tuple(self._gm[name][r].cpu().numpy() for name in ("w", "mu", "cov"))

    def gmm_counts(self) -> np.ndarray:
        """The member counts [k] of the predicted labels; the stable grouping behind them stays on the device for ``gmm_pick``."""
        import torch

        k = int(self._gm["w"].shape[1])
        grouped, self._gm_perm = torch.sort(self._gm_pred, stable=True)  # position order kept inside a component
        self._gm_starts = torch.searchsorted(grouped, torch.arange(k + 1, dtype=torch.int32, device=grouped.device))
        return (self._gm_starts[1:] - self._gm_starts[:-1]).cpu().numpy()

    def gmm_pick(self, components, t) -> np.ndarray:
        """The positions of the ``t[i]``-th member, in position order, of the components ``components[i]``."""
        return self._gm_perm[self._gm_starts[self._index(components)] + self._index(t)].cpu().numpy()


_rows_factory = DeviceRows


def _random_state(seed):
    """``sklearn.utils.check_random_state``."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def _check_nonnegative_int(value, desc, strict=True):
    negative = (value is None) or (value <= 0 if strict else value < 0)
    if negative or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{desc} should be a nonnegative integer. {value} was given")


def _validate(n_clusters, max_iter, init, method, metric):
    """``KMedoids._check_init_args`` in its order and words (kmedoids.py:168-203), then what the HIP path leaves out."""
    _check_nonnegative_int(n_clusters, "n_clusters")
    _check_nonnegative_int(max_iter, "max_iter", False)
    if not (hasattr(init, "__array__") or (isinstance(init, str) and init in _INIT_METHODS)):
        raise ValueError("init needs to be one of " + "the following: " + "%s" % (_INIT_METHODS + ["array-like"]))
    if hasattr(init, "__array__"):
        raise ValueError("An array-like init is not available on the HIP path; use 'k-medoids++' or 'random'.")
    if init in ("heuristic", "build"):
        raise ValueError(f"init='{init}' is not available on the HIP path (its argpartition / BUILD orders on tied sums are not a "
                         f"contract); use 'k-medoids++' or 'random'.")
    if method == "pam":
        raise ValueError("method='pam' is not available on the HIP path; use 'alternate'.")
    if method != "alternate":
        raise ValueError(f"method={method} is not supported. Supported methods are 'pam' and 'alternate'.")
    if metric != "euclidean":
        raise ValueError(f"metric='{metric}' is not available on the HIP path; only 'euclidean' is.")


def _kpp_init(dev, k: int, rs) -> np.ndarray:
    """``KMedoids._kpp_init`` (kmedoids.py:438-511) on rows of the distance matrix computed on demand."""
    n = dev.m
    centers = np.empty(k, dtype=np.int64)
    trials = 2 + int(np.log(k))
    centers[0] = rs.randint(n)
    row = dev.dist_rows(centers[:1])[0]
    closest = row * row
    pot = np.cumsum(closest)[-1]
    for c in range(1, k):
        rand_vals = rs.random_sample(trials) * pot
        cand = np.searchsorted(np.cumsum(closest), rand_vals)
        np.clip(cand, None, n - 1, out=cand)
        rows = dev.dist_rows(cand)
        best = best_pot = best_closest = None
        for t in range(trials):
            new = np.minimum(closest, rows[t] * rows[t])
            new_pot = np.cumsum(new)[-1]
            if best is None or new_pot < best_pot:
                best, best_pot, best_closest = cand[t], new_pot, new
        centers[c], pot, closest = best, best_pot, best_closest
    return centers


def _cluster(dev, n_clusters: int, max_iter: int = 100, init="k-medoids++", random_state=None, method="alternate", metric="euclidean"):
    """``KMedoids(...).fit`` on the selected rows of ``dev``: (medoids, labels, inertia, n_iter)."""
    rs = _random_state(random_state)
    _validate(n_clusters, max_iter, init, method, metric)
    if n_clusters > dev.m:
        raise ValueError("The number of medoids (%d) must be less than the number of samples %d." % (n_clusters, dev.m))
    if init == "random":
        medoids = np.asarray(rs.choice(dev.m, n_clusters, replace=False), dtype=np.int64)
    else:
        medoids = _kpp_init(dev, n_clusters, rs)
    n_iter = 0
    for n_iter in range(max_iter):
        medoids, empty, changed = dev.step(medoids)
        for c in empty:
            warnings.warn("Cluster {k} is empty! self.labels_[self.medoid_indices_[{k}]] may not be labeled with its corresponding "
                          "cluster ({k}).".format(k=c))
        if not changed:
            break
        elif n_iter == max_iter - 1:
            warnings.warn("Maximum number of iteration reached before convergence. Consider increasing max_iter to improve the fit.",
                          ConvergenceWarning)
    labels, dist = dev.assign(medoids)
    return medoids, labels, float(np.sum(dist)), n_iter


def k_medoids(points: np.ndarray, n_clusters: int, max_iter: int = 100, init="k-medoids++", random_state=None, *, device: int = 0,
              return_info: bool = False, method: str = "alternate", metric: str = "euclidean"):
    """The reference's ``KMedoids(n_clusters, init=init, max_iter=max_iter, random_state=random_state).fit(points)`` on the device: the
    medoid positions in cluster order (``medoid_indices_``).  With ``return_info`` also ``labels_``, ``inertia_`` and ``n_iter_``."""
    _validate(n_clusters, max_iter, init, method, metric)  # refused before anything goes to the device
    values = _as_points(points, _MAX_D)
    if n_clusters > values.shape[0]:
        raise ValueError("The number of medoids (%d) must be less than the number of samples %d." % (n_clusters, values.shape[0]))
    rs = _random_state(random_state)
    d = values.shape[1]
    dev = _rows_factory(values, np.zeros(d), np.ones(d), device)  # (x - 0) / 1: the points themselves, bit for bit
    medoids, labels, inertia, n_iter = _cluster(dev, n_clusters, max_iter, init, rs, method, metric)
    medoids = [int(i) for i in medoids]
    return (medoids, labels, inertia, n_iter) if return_info else medoids


def _candidate_positions(labels: pd.Index, candidates_exp: pd.DataFrame):
    """The positions of the candidates, in their own row order (clustering.py:115-116), in the resident matrix whose rows carry
    ``labels``; ``None`` if the candidates are all of its rows in its order."""
    if len(candidates_exp) == len(labels) and candidates_exp.index.equals(labels):
        return None
    pos = labels.get_indexer(candidates_exp.index)
    if (pos < 0).any():
        raise KeyError("candidates contain rows that are not part of the discrete subspace")
    return pos


def _as_points(points, max_d=None, min_rows: int = 1) -> np.ndarray:
    """``points`` as a contiguous fp64 matrix, refused in the words of the public functions: not two-dimensional or too few rows /
    columns, then (``max_d`` given) beyond the limits of the HIP path."""
    values = np.ascontiguousarray(points, dtype=np.float64)
    if values.ndim != 2 or values.shape[0] < min_rows or values.shape[1] < 1:
        need = "at least one row and one column" if min_rows else "at least one column"
        raise ValueError(f"Expected a 2D array with {need}, got an array of shape {values.shape}.")
    if max_d is not None and (values.shape[1] > max_d or values.shape[0] >= _MAX_ROWS):
        raise ValueError(f"The HIP path takes at most {max_d} columns and fewer than 2^31 - 256 rows, got {values.shape}.")
    return values


def _recommender_fields(default_params: dict, check) -> dict:
    """attrs fields of a clustering recommender: the reference's ``model_params`` plus the device and the cache."""
    return {
        "model_params": field(default=attrs.Factory(lambda: dict(default_params)), validator=[instance_of(dict), check]),
        "device": field(default=0, validator=instance_of(int), kw_only=True),
        "_fps_cache": field(default=None, init=False, eq=False, repr=False),
    }


class HipPAMRecommenderImpl(HipFPSRecommenderImpl):
    """Behaviour of the k-medoids recommender on an MI355X.  No fields (see ``baybe_amd.plugin``): they are attached by
    ``attrs.make_class`` - below for the stand-alone class, in ``plugin.make_baybe_pam_recommender`` on top of BayBE's
    ``NonPredictiveRecommender``, whose ``recommend`` then drives ``_recommend_discrete``.  Copying, pickling and the cache key are
    the FPS recommender's."""

    __slots__ = ()

    _SHARED_ON_COPY: ClassVar[tuple] = ("_fps_cache",)

    def _resident_rows(self, subspace_discrete):
        """(rows, labels): the comp rep of the WHOLE discrete subspace with the scaling fitted on it, resident per search-space
        content and device; later calls send only the candidates' positions."""
        from baybe_amd.recommenders import _content_hash, _frame_content_hash

        comp_rep = subspace_discrete.comp_rep
        idx = comp_rep.index
        idx_key = (idx.start, idx.stop, idx.step) if isinstance(idx, pd.RangeIndex) else _content_hash(np.asarray(idx))
        key = (comp_rep.shape, tuple(comp_rep.columns), _frame_content_hash(comp_rep), idx_key, self.device)
        if self._fps_cache is None or self._fps_cache[0] != key:
            values = np.ascontiguousarray(comp_rep.to_numpy(dtype=np.float64))
            mean, scale = standard_scaling(values)  # fitted on the entire search space (nonpredictive/clustering.py:107-112)
            self._fps_cache = (key, _rows_factory(values, mean, scale, self.device), comp_rep.index)
        return self._fps_cache[1], self._fps_cache[2]

    def _recommend_discrete(self, subspace_discrete, candidates_exp: pd.DataFrame, batch_size: int) -> pd.Index:
        dev, labels = self._resident_rows(subspace_discrete)
        dev.select(_candidate_positions(labels, candidates_exp))
        medoids, _, _, _ = _cluster(dev, batch_size, **self.model_params)
        return candidates_exp.index[np.asarray(medoids, dtype=np.int64)]

    def __str__(self) -> str:
        return f"{self.__class__.__name__}(model_params={self.model_params!r})"


def _check_model_params(instance, attribute, value):
    unknown = set(value) - {"max_iter", "init", "random_state", "method", "metric"}
    if unknown:
        raise TypeError(f"KMedoids got unexpected model parameters: {sorted(unknown)}")


def pam_recommender_fields() -> dict:
    """The reference's default (nonpredictive/clustering.py:159-165)."""
    return _recommender_fields({"max_iter": 100, "init": "k-medoids++"}, _check_model_params)


class _StandAlonePAM(HipPAMRecommenderImpl, _StandAloneFPS):
    """``recommend`` of the stand-alone FPS recommender (the refusals and warnings of ``NonPredictiveRecommender.recommend`` /
    ``PureRecommender.recommend``) over the k-medoids ``_recommend_discrete``."""

    __slots__ = ()


HipPAMClusteringRecommender = attrs.make_class("HipPAMClusteringRecommender", pam_recommender_fields(), bases=(_StandAlonePAM,), slots=False)
HipPAMClusteringRecommender.__doc__ = "Initial recommender selecting the medoids of a k-medoids clustering on an MI355X (stand-alone)."
HipPAMClusteringRecommender.__module__ = __name__
HipPAMClusteringRecommender.compatibility = "DISCRETE"


# ---- k-means ---------------------------------------------------------------------------------------------------------------------
def _is_int(value) -> bool:
    return isinstance(value, (int, np.integer)) and not isinstance(value, bool)


def _validate_kmeans(n_clusters, n_init, max_iter, tol, init, algorithm, sample_weight=None):
    """scikit-learn's parameter validation in its words (``sklearn/utils/_param_validation.py``), then what the HIP path leaves out."""
    if not (_is_int(n_clusters) and n_clusters >= 1):
        raise ValueError(f"The 'n_clusters' parameter of KMeans must be an int in the range [1, inf). Got {n_clusters!r} instead.")
    if not (_is_int(max_iter) and max_iter >= 1):
        raise ValueError(f"The 'max_iter' parameter of KMeans must be an int in the range [1, inf). Got {max_iter!r} instead.")
    if not ((isinstance(n_init, str) and n_init == "auto") or (_is_int(n_init) and n_init >= 1)):
        raise ValueError(f"The 'n_init' parameter of KMeans must be a str among {{'auto'}} or an int in the range [1, inf). "
                         f"Got {n_init!r} instead.")
    if not (isinstance(tol, (int, float, np.integer, np.floating)) and not isinstance(tol, bool) and tol >= 0):
        raise ValueError(f"The 'tol' parameter of KMeans must be a float in the range [0.0, inf). Got {tol!r} instead.")
    if callable(init) or hasattr(init, "__array__") or isinstance(init, (list, tuple)):
        raise ValueError("An array-like or callable init is not available on the HIP path; use 'k-means++' or 'random'.")
    if not (isinstance(init, str) and init in ("k-means++", "random")):
        raise ValueError(f"init needs to be 'k-means++' or 'random'. Got {init!r} instead.")
    if algorithm == "elkan":
        raise ValueError("algorithm='elkan' is not available on the HIP path; use 'lloyd'.")
    if algorithm != "lloyd":
        raise ValueError(f"algorithm needs to be 'lloyd' or 'elkan'. Got {algorithm!r} instead.")
    if sample_weight is not None:
        raise ValueError("Sample weights are not available on the HIP path.")


def _same_clustering(labels, best, k: int) -> bool:
    """``sklearn.cluster._k_means_common._is_same_clustering``: every label of ``labels`` meets a single label of ``best``."""
    pairs = np.unique(labels.astype(np.int64) * k + best)
    return len(np.unique(pairs // k)) == len(pairs)


def _kmeans_run(dev, n_clusters: int, n_init="auto", max_iter: int = 300, tol: float = 1e-4, init="k-means++", random_state=None,
                algorithm="lloyd"):
    """Every restart of the contract of the module docstring on the selected rows of ``dev``, side by side: (inertia [R], n_iter
    [R]); the restarts' labels and centres stay on ``dev``."""
    rs = _random_state(random_state)
    N, k = dev.m, n_clusters
    if k > N:
        raise ValueError(f"n_samples={N} should be >= n_clusters={k}.")
    R = (1 if init == "k-means++" else 10) if isinstance(n_init, str) else int(n_init)
    if init == "random":
        idx = np.stack([np.asarray(rs.choice(N, k, replace=False), dtype=np.int64) for _ in range(R)])
    else:
        idx = _kpp_positions(dev, k, R, rs)
    dev.kmeans_begin(idx)
    threshold = tol * dev.mean_variance()
    active = list(range(R))
    n_iter, strict = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=bool)
    for _ in range(max_iter):
        if not active:
            break
        same, shift = dev.kmeans_step(active)  # every still-running restart in one pass
        n_iter[active] += 1
        strict[np.asarray(active)[same]] = True
        active = [r for a, r in enumerate(active) if not same[a] and not shift[a] <= threshold]
    return dev.kmeans_finish([r for r in range(R) if not strict[r]]), n_iter


def _kpp_positions(dev, k: int, R: int, rs) -> np.ndarray:
    """The k-means++ centre positions [R, k] of R restarts from ``rs.random_sample((R, 1 + (k - 1) T))``."""
    N = dev.m
    T = 2 + int(np.log(k))
    U = rs.random_sample((R, 1 + (k - 1) * T))
    cdf = np.cumsum(np.full(N, 1.0 / N))
    cdf /= cdf[-1]
    first = np.minimum(np.searchsorted(cdf, U[:, 0], side="right"), N - 1).astype(np.int64)
    return dev.kmeans_seed(first, U[:, 1:], k)


def _kmeans_fit(dev, n_clusters: int, n_init="auto", max_iter: int = 300, tol: float = 1e-4, init="k-means++", random_state=None,
                algorithm="lloyd"):
    """The contract of the module docstring on the selected rows of ``dev``: (centres, labels, inertia, n_iter, winning restart)."""
    k = n_clusters
    inertia, n_iter = _kmeans_run(dev, n_clusters, n_init, max_iter, tol, init, random_state, algorithm)
    R = len(inertia)
    best, best_labels = 0, dev.kmeans_labels(0)
    for r in range(1, R):
        if inertia[r] < inertia[best]:
            labels = dev.kmeans_labels(r)
            if not _same_clustering(labels, best_labels, k):
                best, best_labels = r, labels
    distinct = len(np.unique(best_labels))
    if distinct < k:
        warnings.warn(f"Number of distinct clusters ({distinct}) found smaller than n_clusters ({k}). Possibly due to duplicate points "
                      f"in X.", ConvergenceWarning, stacklevel=2)
    return dev.kmeans_centres(best), best_labels, float(inertia[best]), int(n_iter[best]), best


def k_means(points: np.ndarray, n_clusters: int, *, n_init="auto", max_iter: int = 300, tol: float = 1e-4, init="k-means++",
            random_state=None, algorithm: str = "lloyd", device: int = 0, return_info: bool = False, sample_weight=None):
    """``sklearn.cluster.KMeans(n_clusters, n_init=n_init, max_iter=max_iter, tol=tol, init=init, random_state=random_state)
    .fit(points)`` on the device, all restarts as one workload: ``cluster_centers_`` [k, d].  With ``return_info`` also ``labels_``,
    ``inertia_`` and ``n_iter_``.  ``n_init="auto"``: 1 for k-means++, 10 for random."""
    _validate_kmeans(n_clusters, n_init, max_iter, tol, init, algorithm, sample_weight)  # refused before anything goes to the device
    values = _as_points(points, _MAX_D)
    if n_clusters > values.shape[0]:
        raise ValueError(f"n_samples={values.shape[0]} should be >= n_clusters={n_clusters}.")
    rs = _random_state(random_state)
    d = values.shape[1]
    dev = _rows_factory(values, np.zeros(d), np.ones(d), device)  # (x - 0) / 1: the points themselves, bit for bit
    centres, labels, inertia, n_iter, _ = _kmeans_fit(dev, n_clusters, n_init, max_iter, tol, init, rs, algorithm)
    return (centres, labels, inertia, n_iter) if return_info else centres


class HipKMeansRecommenderImpl(HipPAMRecommenderImpl):
    """Behaviour of the k-means recommender on an MI355X, built like the k-medoids one: the resident matrix, its cache key, copying
    and pickling are shared; the clustering is ``_kmeans_fit`` and the selection the reference's (the member nearest to each
    centre)."""

    __slots__ = ()

    def _recommend_discrete(self, subspace_discrete, candidates_exp: pd.DataFrame, batch_size: int) -> pd.Index:
        params = {"n_init": "auto", "max_iter": 300, "tol": 1e-4, "init": "k-means++", "algorithm": "lloyd", **self.model_params}
        _validate_kmeans(batch_size, params["n_init"], params["max_iter"], params["tol"], params["init"], params["algorithm"])
        dev, labels = self._resident_rows(subspace_discrete)
        dev.select(_candidate_positions(labels, candidates_exp))
        centres, _, _, _, _ = _kmeans_fit(dev, batch_size, **params)
        return candidates_exp.index[np.asarray(dev.kmeans_select(centres), dtype=np.int64)]


def _check_kmeans_model_params(instance, attribute, value):
    unknown = set(value) - {"n_init", "max_iter", "tol", "init", "random_state", "algorithm"}
    if unknown:
        raise TypeError(f"KMeans got unexpected model parameters: {sorted(unknown)}")


def kmeans_recommender_fields() -> dict:
    """The reference's default (nonpredictive/clustering.py:207-214)."""
    return _recommender_fields({"max_iter": 1000, "n_init": 50}, _check_kmeans_model_params)


class _StandAloneKMeans(HipKMeansRecommenderImpl, _StandAloneFPS):
    """``recommend`` of the stand-alone FPS recommender over the k-means ``_recommend_discrete``."""

    __slots__ = ()


HipKMeansClusteringRecommender = attrs.make_class("HipKMeansClusteringRecommender", kmeans_recommender_fields(), bases=(_StandAloneKMeans,),
                                                  slots=False)
HipKMeansClusteringRecommender.__doc__ = ("Initial recommender selecting the member nearest to each centre of a k-means clustering on an "
                                          "MI355X (stand-alone).")
HipKMeansClusteringRecommender.__module__ = __name__
HipKMeansClusteringRecommender.compatibility = "DISCRETE"


# ---- Gaussian mixture ------------------------------------------------------------------------------------------------------------
_GMM_MAX_D = 64
_GMM_MAX_K = 65535  # a grid dimension of the M-step and of the precision factor
_COVARIANCE_TYPES = ("full", "tied", "diag", "spherical")
_INIT_PARAMS = ("kmeans", "random", "random_from_data", "k-means++")
_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
                "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.")
_NOT_CONVERGED = ("Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or check "
                  "for degenerate data.")


def _is_real(value) -> bool:
    return isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool)


def _validate_gmm(n_components, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params="kmeans",
                  weights_init=None, means_init=None, precisions_init=None, warm_start=False, shape=None):
    """scikit-learn's parameter validation in its words and its (alphabetical) order, its two checks of the sample count, then what
    the HIP path leaves out."""
    def among(options):
        return "{" + ", ".join(repr(o) for o in options) + "}"

    if not (isinstance(covariance_type, str) and covariance_type in _COVARIANCE_TYPES):
        raise ValueError(f"The 'covariance_type' parameter of GaussianMixture must be a str among {among(_COVARIANCE_TYPES)}. "
                         f"Got {covariance_type!r} instead.")
    if not (isinstance(init_params, str) and init_params in _INIT_PARAMS):
        raise ValueError(f"The 'init_params' parameter of GaussianMixture must be a str among {among(_INIT_PARAMS)}. "
                         f"Got {init_params!r} instead.")
    if not (_is_int(max_iter) and max_iter >= 0):
        raise ValueError(f"The 'max_iter' parameter of GaussianMixture must be an int in the range [0, inf). Got {max_iter!r} instead.")
    if not (_is_int(n_components) and n_components >= 1):
        raise ValueError(f"The 'n_components' parameter of GaussianMixture must be an int in the range [1, inf). "
                         f"Got {n_components!r} instead.")
    if not (_is_int(n_init) and n_init >= 1):
        raise ValueError(f"The 'n_init' parameter of GaussianMixture must be an int in the range [1, inf). Got {n_init!r} instead.")
    if not (_is_real(reg_covar) and reg_covar >= 0):
        raise ValueError(f"The 'reg_covar' parameter of GaussianMixture must be a float in the range [0.0, inf). Got {reg_covar!r} instead.")
    if not (_is_real(tol) and tol >= 0):
        raise ValueError(f"The 'tol' parameter of GaussianMixture must be a float in the range [0.0, inf). Got {tol!r} instead.")
    if shape is not None:
        if shape[0] < 2:
            raise ValueError(f"Found array with {shape[0]} sample(s) (shape={tuple(shape)}) while a minimum of 2 is required by "
                             f"GaussianMixture.")
        if shape[0] < n_components:
            raise ValueError(f"Expected n_samples >= n_components but got n_components = {n_components}, n_samples = {shape[0]}")
    if covariance_type != "full":
        raise ValueError(f"covariance_type='{covariance_type}' is not available on the HIP path; only 'full' is.")
    if init_params == "random":
        raise ValueError("init_params='random' is not available on the HIP path (it needs an [N, k] upload); use 'kmeans', 'k-means++' "
                         "or 'random_from_data'.")
    if weights_init is not None or means_init is not None or precisions_init is not None:
        raise ValueError("weights_init, means_init and precisions_init are not available on the HIP path.")
    if warm_start:
        raise ValueError("warm_start is not available on the HIP path.")
    if shape is not None and shape[1] > _GMM_MAX_D:
        raise ValueError(f"The HIP path takes at most {_GMM_MAX_D} columns for full covariances, got {shape[1]}; wider comp reps go to "
                         f"k-means.")
    if n_components > _GMM_MAX_K:
        raise ValueError(f"The HIP path takes at most {_GMM_MAX_K} components, got {n_components}.")


def _gmm_fit(dev, n_components: int, covariance_type="full", tol: float = 1e-3, reg_covar: float = 1e-6, max_iter: int = 100,
             n_init: int = 1, init_params="kmeans", random_state=None):
    """The Gaussian mixture contract of the module docstring on the selected rows of ``dev``: (weights, means, covariances, lower bound,
    n_iter, converged, winning restart).  The winner's labels are predicted on ``dev`` (``dev.gmm_labels()``, ``_gmm_select``)."""
    rs = _random_state(random_state)
    N, k, R = dev.m, n_components, int(n_init)
    _validate_gmm(k, covariance_type, tol, reg_covar, max_iter, R, init_params, shape=(N, dev.d))
    if init_params == "kmeans":
        _kmeans_run(dev, k, R, 300, 1e-4, "k-means++", rs)
        distinct, flags, G = dev.gmm_begin(k, reg_covar)
        for r in range(R):  # scikit-learn's warning, per restart
            if distinct[r] < k:
                warnings.warn(f"Number of distinct clusters ({distinct[r]}) found smaller than n_clusters ({k}). Possibly due to "
                              f"duplicate points in X.", ConvergenceWarning, stacklevel=2)
    else:
        if init_params == "k-means++":
            idx = _kpp_positions(dev, k, R, rs)
        else:
            idx = np.stack([np.asarray(rs.choice(N, k, replace=False), dtype=np.int64) for _ in range(R)])
        _, flags, G = dev.gmm_begin(k, reg_covar, idx)
    if flags.any():
        raise ValueError(_ILL_DEFINED)
    lower, n_iter, converged = np.full(R, -np.inf), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=bool)
    for base in range(0, R, G):  # the restarts of a group share log_resp
        active = list(range(base, min(base + G, R)))
        for _ in range(max_iter):
            if not active:
                break
            lb, flags = dev.gmm_step(active, base)  # every still-running restart of the group in one pass
            if flags.any():
                raise ValueError(_ILL_DEFINED)
            act = np.asarray(active)
            change = lb - lower[act]
            lower[act] = lb
            n_iter[act] += 1
            done = np.abs(change) < tol
            converged[act[done]] = True
            active = [r for a, r in enumerate(active) if not done[a]]
    best = -1
    for r in range(R):
        if best < 0 or lower[r] > lower[best]:
            best = r
    if not converged[best] and max_iter > 0:
        warnings.warn(_NOT_CONVERGED, ConvergenceWarning, stacklevel=2)
    dev.gmm_predict(best)
    weights, means, covariances = dev.gmm_result(best)
    return weights, means, covariances, float(lower[best]), int(n_iter[best]), bool(converged[best]), best


def _gmm_select(dev) -> np.ndarray:
    """The reference's ``_make_selection_default`` (``nonpredictive/clustering.py:55-76``) on the labels ``dev`` predicted: one
    ``np.random.choice`` among the members of every non-empty component, ascending - the global generator, consumed as the reference
    consumes it.  Positions, fewer than the number of components if one is empty."""
    counts = dev.gmm_counts()
    components = np.flatnonzero(counts > 0)
    t = np.array([np.random.choice(int(counts[c])) for c in components], dtype=np.int64)
    return np.asarray(dev.gmm_pick(components, t), dtype=np.int64)


def gaussian_mixture(points: np.ndarray, n_components: int, *, covariance_type="full", tol: float = 1e-3, reg_covar: float = 1e-6,
                     max_iter: int = 100, n_init: int = 1, init_params="kmeans", random_state=None, weights_init=None, means_init=None,
                     precisions_init=None, warm_start: bool = False, device: int = 0, return_info: bool = False):
    """``sklearn.mixture.GaussianMixture(n_components, ...).fit(points)`` on the device, all restarts as one workload: ``(weights_,
    means_, covariances_)``.  With ``return_info`` also the labels of ``predict(points)``, ``lower_bound_``, ``n_iter_`` and
    ``converged_``."""
    values = _as_points(points, min_rows=0)
    _validate_gmm(n_components, covariance_type, tol, reg_covar, max_iter, n_init, init_params, weights_init, means_init, precisions_init,
                  warm_start, values.shape)  # refused before anything goes to the device
    if values.shape[0] >= _MAX_ROWS:
        raise ValueError(f"The HIP path takes fewer than 2^31 - 256 rows, got {values.shape}.")
    rs = _random_state(random_state)
    d = values.shape[1]
    dev = _rows_factory(values, np.zeros(d), np.ones(d), device)  # (x - 0) / 1: the points themselves, bit for bit
    weights, means, covariances, lower, n_iter, converged, _ = _gmm_fit(dev, n_components, covariance_type, tol, reg_covar, max_iter,
                                                                        n_init, init_params, rs)
    if return_info:
        return weights, means, covariances, dev.gmm_labels(), lower, n_iter, converged
    return weights, means, covariances


class HipGMMRecommenderImpl(HipPAMRecommenderImpl):
    """Behaviour of the Gaussian mixture recommender on an MI355X, built like the k-medoids one: the resident matrix, its cache key,
    copying and pickling are shared; the clustering is ``_gmm_fit`` and the selection the reference's default one (a random member
    of every non-empty component).  A component without members yields no row, so fewer than ``batch_size`` rows can come back, as
    from the reference."""

    __slots__ = ()

    def _recommend_discrete(self, subspace_discrete, candidates_exp: pd.DataFrame, batch_size: int) -> pd.Index:
        params = dict(self.model_params)
        extra = {name: params.pop(name) for name in ("weights_init", "means_init", "precisions_init", "warm_start") if name in params}
        _validate_gmm(batch_size, **{n: params[n] for n in params if n != "random_state"}, **extra,
                      shape=(len(candidates_exp), subspace_discrete.comp_rep.shape[1]))
        dev, labels = self._resident_rows(subspace_discrete)
        dev.select(_candidate_positions(labels, candidates_exp))
        _gmm_fit(dev, batch_size, **params)
        return candidates_exp.index[_gmm_select(dev)]


def _check_gmm_model_params(instance, attribute, value):
    unknown = set(value) - {"covariance_type", "tol", "reg_covar", "max_iter", "n_init", "init_params", "random_state", "weights_init",
                            "means_init", "precisions_init", "warm_start"}
    if unknown:
        raise TypeError(f"GaussianMixture got unexpected model parameters: {sorted(unknown)}")


def gmm_recommender_fields() -> dict:
    """The reference's default (nonpredictive/clustering.py:263-268)."""
    return _recommender_fields({}, _check_gmm_model_params)


class _StandAloneGMM(HipGMMRecommenderImpl, _StandAloneFPS):
    """``recommend`` of the stand-alone FPS recommender over the Gaussian mixture ``_recommend_discrete``."""

    __slots__ = ()


HipGaussianMixtureClusteringRecommender = attrs.make_class("HipGaussianMixtureClusteringRecommender", gmm_recommender_fields(),
                                                           bases=(_StandAloneGMM,), slots=False)
HipGaussianMixtureClusteringRecommender.__doc__ = ("Initial recommender selecting a random member of every component of a Gaussian "
                                                   "mixture clustering on an MI355X (stand-alone).")
HipGaussianMixtureClusteringRecommender.__module__ = __name__
HipGaussianMixtureClusteringRecommender.compatibility = "DISCRETE"
