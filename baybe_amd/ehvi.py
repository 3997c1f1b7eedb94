"""qExpectedHypervolumeImprovement / qLogExpectedHypervolumeImprovement (``baybe/acquisition/acqfs.py:429-464``) on the HIP path.

The non-noisy pair of the hypervolume family.  Unlike qLogNEHVI / qNEHVI (``baybe_amd.nehvi``) the partitioning is built ONCE per
recommendation - from the oriented posterior means of every target's model at ALL measurement rows (``_posterior_mean_comp``,
``baybe/acquisition/_builder.py:195-317``; ``make_partitioning``, ``baybe/acquisition/utils.py:26-84``) - and pending points are
not cached into a baseline: ``optimize_acqf_discrete`` concatenates earlier picks and ``pending_experiments`` to every candidate
(``X_pending``), so each candidate scores the joint batch ``[x_i ; pending]`` of q' = 1 + p points by inclusion-exclusion over its
subsets (``csrc/bbh_ehvi.hip``; the estimators are restated in ``tests/_oracle_ehvi.py``).  [UPSTREAM] BoTorch is restated from
memory, parity unpinned: ``alpha=None`` is BoTorch's default, 0 for up to 4 objectives; ``alpha == 0`` is the exact
``FastNondominatedPartitioning``, the decomposition of ``baybe_amd.box_decomposition``; the approximate partitioning of
``alpha > 0`` is a different algorithm and is refused.

``HipEHVI`` has the shape of ``HipDesirability``: the m posterior passes stay resident as ``[m, N]`` through a greedy batch, every
step adds the picks' cross-covariances and pending statistics per target, and one ``ehvi_acq`` call scores all candidates.  The
kernels take ORIENTED operands: the means (and pending means) of a minimised target are negated here, and so is that target's
base-sample column - sign (m + L z) = (sign m) + L (sign z) - while variances and covariances carry no sign."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from baybe_amd.engine import GreedyResult, draw_sampler_seed, sobol_normal_base_samples
from baybe_amd.exceptions import IncompatibilityError
from baybe_amd.scoring import refuse_shard

MAX_OBJECTIVES = 4  # BBH_MAX_OBJECTIVES


def shard_text(name: str) -> str:
    return (f"Row shards are not on the HIP path of '{name}'; score the candidates on one device, or use "
            f"qLogNoisyExpectedHypervolumeImprovement.")


def check_alpha(alpha) -> None:
    """The alpha rule, checked before anything is fitted: None (BoTorch's default, 0 for up to 4 objectives) and 0 are the exact
    partitioning; a positive alpha asks for BoTorch's approximate ``NondominatedPartitioning``."""
    if alpha is not None and float(alpha) != 0.0:
        raise IncompatibilityError(
            f"alpha={alpha!r} asks for BoTorch's approximate NondominatedPartitioning, which is not on the HIP path; use alpha=0 "
            f"(the exact partitioning, also the default for up to {MAX_OBJECTIVES} targets) or BotorchRecommender."
        )


def make_partitioning(means, ref, alpha=None):
    """``baybe.acquisition.utils.make_partitioning``: (lower [C, m], upper [C, m]) of the disjoint boxes that tile the region above
    ``ref`` not dominated by the rows of ``means`` [n, m] (both oriented: larger is better); upper bounds may be +inf."""
    from baybe_amd.box_decomposition import nondominated_cells

    means, ref = np.asarray(means, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if means.ndim != 2:
        raise ValueError(f"Predictions must be a 2-D tensor, got shape {means.shape}.")
    if ref.ndim != 1:
        raise ValueError(f"Reference point must be a 1-D tensor, got shape {ref.shape}.")
    if (n_p := means.shape[1]) != (n_r := len(ref)):
        raise ValueError(f"Predictions dimensionality {n_p} does not match reference point dimensionality {n_r}.")
    check_alpha(alpha)
    if not 2 <= n_r <= MAX_OBJECTIVES:
        raise IncompatibilityError(
            f"The HIP path scores hypervolume improvements of 2 to {MAX_OBJECTIVES} targets ({n_r} given). Use BotorchRecommender.")
    lo, up = nondominated_cells(means, ref)
    return np.ascontiguousarray(lo), np.ascontiguousarray(up)


class HipEHVI:
    """qEHVI (``log=False``) / qLogEHVI values over m independent HIP GPs: ``cells`` / ``score`` / ``greedy`` / ``joint_value``.
    Every call that reaches the device goes through the engines (``posterior``, ``set_pending``, ``cross_cov``, ``argmax``, and the
    first engine's ``ehvi_acq``)."""

    def __init__(self, engines, signs, X_all, ref_point, log: bool = True, n_mc_samples: int = 128, alpha=None, device: int = 0):
        self.engines = list(engines)
        self.signs = np.asarray(signs, dtype=np.float64).reshape(-1)
        if len(self.engines) != len(self.signs):
            raise ValueError(f"{len(self.signs)} targets need as many models, got {len(self.engines)}")
        self.outputs = [SimpleNamespace(engine=e, ext=e) for e in self.engines]
        self.ref = np.asarray(ref_point, dtype=np.float64).reshape(-1)
        self.log, self.S, self.alpha, self.device = bool(log), int(n_mc_samples), alpha, int(device)
        self.X_all = np.ascontiguousarray(np.atleast_2d(X_all), dtype=np.float64)
        self._cells = None

    @property
    def m(self) -> int:
        return len(self.engines)

    def cells(self):
        """(lower, upper) [C, m]: the partitioning of the models' oriented posterior means at ALL measurement rows
        (``_posterior_mean_comp``).  Every model is evaluated at all rows: with partial measurements each was trained on its own
        subset."""
        if self._cells is None:
            mu = np.stack([e.posterior(self.X_all)[0].cpu().numpy() for e in self.engines], axis=-1) * self.signs[None, :]  # [n, m]
            self._cells = make_partitioning(mu, self.ref, self.alpha)
        return self._cells

    def base_samples(self, q: int, seed: int) -> np.ndarray:
        """[S, q, m]: one Sobol draw over the q m normal variables (the ``[S, q', T]`` convention of ``desirability.py``)."""
        return sobol_normal_base_samples(self.S, q * self.m, seed).reshape(self.S, q, self.m)

    def _moments(self, X):
        """(X on the device, oriented means [m, N], variances [m, N])."""
        import torch

        X = self.engines[0]._as_dev(X)
        pairs = []
        for e in self.engines:
            e.set_pending(None)
            pairs.append(e.posterior(X))
        sign = torch.as_tensor(self.signs, dtype=torch.float64, device=X.device)[:, None]
        return X, (torch.stack([m for m, _ in pairs]) * sign).contiguous(), torch.stack([v for _, v in pairs]).contiguous()

    def _pending_terms(self, X, pend):
        """(cross [m, N, p], (oriented mean_p [m, p], cov_pp [m, p, p])) of the pending rows under every model."""
        import torch

        cross, mps, cpps = [], [], []
        for e in self.engines:
            mp, cpp = e.set_pending(pend)
            cross.append(e.cross_cov(X))
            mps.append(np.asarray(mp, dtype=np.float64)), cpps.append(np.asarray(cpp, dtype=np.float64))
        return torch.stack(cross).contiguous(), (np.stack(mps) * self.signs[:, None], np.stack(cpps))

    def _clear_pending(self):
        for e in self.engines:
            e.set_pending(None)

    def _score(self, X, mean, var, pend, z, alive, form=-1):
        z = np.ascontiguousarray(z, dtype=np.float64) * self.signs  # (the last axis is the target)
        if pend is None or len(pend) == 0:
            return self.engines[0].ehvi_acq(self.log, mean, var, self.cells(), z[:, 0, :], alive)
        cross, stats = self._pending_terms(X, pend)
        return self.engines[0].ehvi_acq(self.log, mean, var, self.cells(), z, alive, cross=cross, stats=stats, form=form)

    @staticmethod
    def check_batch(n_points: int) -> None:
        """1 + pending + picks must fit the kernels' joint batch."""
        from baybe_amd import _lib

        if n_points > _lib.EHVI_MAX_Q:
            raise IncompatibilityError(
                f"qEHVI / qLogEHVI score the candidate jointly with the pending experiments and the batch's earlier picks by "
                f"inclusion-exclusion over their subsets; {n_points} points exceed the HIP kernels' limit of {_lib.EHVI_MAX_Q}. Use "
                f"qLogNEHVI (qLogNoisyExpectedHypervolumeImprovement), which caches pending points into its baseline and has no such "
                f"limit, or BotorchRecommender."
            )

    def score(self, X, X_pending=None, z=None, seed=None, alive=None):
        """Acquisition values [N] of the t-batches [x_i ; X_pending]; ``z`` [S, 1 + p, m] or drawn from ``seed``."""
        pend = None if X_pending is None or len(X_pending) == 0 else np.ascontiguousarray(np.atleast_2d(X_pending), dtype=np.float64)
        p = 0 if pend is None else len(pend)
        self.check_batch(1 + p)
        if z is None:
            z = self.base_samples(1 + p, draw_sampler_seed() if seed is None else seed)
        self.cells()  # (before pending points are set: it evaluates the plain posterior)
        X, mean, var = self._moments(X)
        try:
            return self._score(X, mean, var, pend, z, alive)
        finally:
            if p:
                self._clear_pending()

    # ---- the recommender's surface (``baybe_amd.scoring``): ONE sampler seed per call ------------------------------------------
    supports_continuous = False

    @staticmethod
    def check_request(batch_size, n_pend, acqf=None, program=None, model=None) -> None:
        """The candidate, the pending experiments and the picks are ONE joint batch (no baseline to cache them into)."""
        HipEHVI.check_batch(1 + n_pend + batch_size)

    def select(self, X, q, *, seeds, X_pending=None, alive=None, shard=None) -> GreedyResult:
        refuse_shard(shard, shard_text("qLogExpectedHypervolumeImprovement" if self.log else "qExpectedHypervolumeImprovement"))
        return self.greedy(X, q, seed=seeds(), X_pending=X_pending, alive=alive)

    def values(self, X, *, seeds, X_pending=None):
        return self.score(X, X_pending=X_pending, seed=seeds())

    def joint_value(self, batch, *, seeds, X_pending=None) -> float:
        """The value of the whole batch ``[batch ; X_pending]`` as one joint q-batch: its first point scored with the others pending
        (the inclusion-exclusion is symmetric in the points)."""
        batch = np.atleast_2d(np.asarray(batch, dtype=np.float64))
        rest = batch[1:] if X_pending is None or len(X_pending) == 0 else np.vstack([batch[1:], np.atleast_2d(X_pending)])
        return float(self.score(batch[:1], X_pending=rest, seed=seeds()).cpu().numpy()[0])

    def greedy(self, X, q: int, seed=None, X_pending=None, alive=None) -> GreedyResult:
        """Sequential greedy of ``optimize_acqf_discrete``: the m posterior passes once, then per step the picks' cross-covariances
        and pending statistics per target and one scoring call; first index on ties, picks leave the candidate set."""
        import torch

        seed = draw_sampler_seed() if seed is None else seed
        d = self.engines[0].spec.d
        base = np.zeros((0, d)) if X_pending is None or len(X_pending) == 0 else np.atleast_2d(np.asarray(X_pending, dtype=np.float64))[:, :d]
        self.check_batch(1 + len(base) + q)  # (the recommender's rule, DESIGN.md section 8: one point of headroom over the last step's q')
        self.cells()
        X, mean, var = self._moments(X)
        N = X.shape[0]
        alive = torch.ones(N, dtype=torch.uint8, device=X.device) if alive is None else alive.clone()
        rows, indices, values = [], [], []
        try:
            for _ in range(q):
                pend = np.vstack([base] + rows) if rows else base
                scores = self._score(X, mean, var, pend, self.base_samples(1 + len(pend), seed), alive)
                val, idx = self.engines[0].argmax(scores)
                indices.append(int(idx)), values.append(float(val))
                alive[idx] = 0
                rows.append(X[idx, :d].cpu().numpy().reshape(1, d))
        finally:
            self._clear_pending()
        return GreedyResult(indices, values)
