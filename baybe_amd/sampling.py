"""Farthest point sampling on the device, and the initial recommender built on it.

``farthest_point_sampling`` mirrors ``baybe/utils/sampling_algorithms.py:15-172`` (same arguments, validation, error texts and
warning) and ``HipFPSRecommenderImpl._recommend_discrete`` mirrors ``FPSRecommender._recommend_discrete``
(``baybe/recommenders/pure/nonpredictive/sampling.py:146-177``), without the N x N distance matrix the reference builds on the host
(80 GB at 1e5 candidates): an all-pairs pass over the resident matrix finds the starting pair, one O(N d) pass per pick does the rest
(``csrc/bbh_fps.hip``).

The arithmetic every comparison rests on is ``d2(x, y) = sum_k (x_k - y_k) * (x_k - y_k)``, k ascending, nothing contracted, and
every tie rule is stated in RANKS (positions in ``np.lexsort(tuple(points.T))``): the farthest pair is the smallest ``a``, then the
smallest ``b``; a pick takes the largest rank among bit-equal maxima, or the ``np.random.choice(count)``-th in rank order.  On points
in generic position this reproduces the reference pick for pick; on grids, where mathematically tied distances are told apart only
by the rounding of sklearn's ``|x|^2 + |y|^2 - 2 x.y`` form, it resolves ties by the rule above instead.
"""

from __future__ import annotations

import warnings
from collections import Counter
from collections.abc import Collection
from typing import ClassVar

import attrs
import numpy as np
import pandas as pd
from attrs import field
from attrs.validators import instance_of

from baybe_amd.exceptions import IncompatibleArgumentError, NotEnoughPointsLeftError, UnusedObjectWarning
from baybe_amd.surrogates import _availability_property

_SCALE_FLOOR = 10 * np.finfo(np.float64).eps  # sklearn's StandardScaler: a smaller scale counts as 1


def standard_scaling(values: np.ndarray):
    """(mean, scale) of ``StandardScaler().fit(values)``: column means and population standard deviations (ddof 0) of the row-major
    matrix (numpy sums in memory order, so the layout decides the last bit: callers pass C-contiguous values)."""
    mean = values.mean(axis=0)
    scale = values.std(axis=0)
    scale[scale < _SCALE_FLOOR] = 1.0
    return mean, scale


class DevicePoints:
    """The scaled points of one matrix, resident on the device in rank order (``P [d, ldp]``), on a model-less ``HipGP`` handle.
    This is the whole device surface of the module: the tests double it on the CPU."""

    def __init__(self, values: np.ndarray, mean: np.ndarray, scale: np.ndarray, device: int = 0):
        import torch

        from baybe_amd.engine import HipGP

        self.gp = HipGP(device)
        self.n, self.d = values.shape
        X = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(self.gp._dev())
        # ranking: np.lexsort(tuple(points.T)) of the SCALED values as successive stable sorts on the device, first column (the least
        # significant key) first; ``+ 0.0`` folds -0.0 into +0.0, which compare equal on the host but not in a radix sort
        unranked = self.gp.fps_prepare(X, mean, scale)
        order = torch.arange(self.n, device=X.device)
        for k in range(self.d):
            order = order[torch.sort(unranked[k, : self.n][order] + 0.0, stable=True).indices]
        del unranked
        self.P = self.gp.fps_prepare(X, mean, scale, order)
        self.order = order.cpu().numpy()  # rank -> row

    def _mask(self, alive_ranked):
        import torch

        return None if alive_ranked is None else torch.from_numpy(alive_ranked.astype(np.uint8)).to(self.P.device)

    def points(self) -> np.ndarray:
        """The scaled points in rank order, [n, d] on the host."""
        return self.P[:, : self.n].T.cpu().numpy()

    def all_identical(self, alive_ranked=None) -> bool:
        cols = self.P[:, : self.n]
        if alive_ranked is not None:
            cols = cols[:, self._mask(alive_ranked).bool()]
        return bool((cols == cols[:, :1]).all().item())

    def farthest_pair(self, alive_ranked=None):
        return self.gp.fps_farthest_pair(self.P, self.n, self._mask(alive_ranked))

    def begin(self, starts, alive_ranked=None, want_count=False) -> int:
        self._alive_dev = self._mask(alive_ranked)  # (kept alive for the calls that continue the selection)
        return self.gp.fps_greedy(self.P, self.n, self._alive_dev, starts=starts, want_count=want_count)[2]

    def picks(self, n_picks: int):
        """``n_picks`` picks, each the LAST of the tied rows: (ranks, d2)."""
        ranks, d2, _ = self.gp.fps_greedy(self.P, self.n, n_picks=n_picks)
        return ranks, d2

    def pick_kth(self, k: int, want_count: bool):
        """One pick, the k-th of the tied rows in rank order: (rank, d2, tie count of the next pick)."""
        ranks, d2, count = self.gp.fps_greedy(self.P, self.n, n_picks=1, k=k, want_count=want_count)
        return int(ranks[0]), float(d2[0]), count


def _select(dp, n_samples: int, initialization, random_tie_break: bool, alive=None):
    """The selection on resident points: (row indices, d2 per pick).  ``alive`` [n] bool in row order or None."""
    alive_ranked = None if alive is None else np.ascontiguousarray(alive[dp.order])
    n_live = dp.n if alive is None else int(alive_ranked.sum())
    if dp.all_identical(alive_ranked):
        warnings.warn("All points are identical.", UserWarning)
        rows = np.arange(dp.n) if alive is None else np.flatnonzero(alive)
        return rows[:n_samples].tolist(), np.zeros(n_samples)
    if isinstance(initialization, str) and initialization == "random":
        r = int(np.random.randint(0, n_live))  # a rank among the live rows (the restriction of the full ranking)
        starts, d2 = [r if alive is None else int(np.flatnonzero(alive_ranked)[r])], [np.inf]
    elif isinstance(initialization, str) and initialization == "farthest":
        v, a, b = dp.farthest_pair(alive_ranked)
        if n_samples == 1:
            return [int(dp.order[a])], np.array([v])
        starts, d2 = [a, b], [v, v]
    else:
        rank_of = np.empty(dp.n, dtype=np.int64)
        rank_of[dp.order] = np.arange(dp.n)
        starts = [int(rank_of[i]) for i in initialization]
        if alive_ranked is not None and not alive_ranked[starts].all():
            raise ValueError("Initialization indices must refer to candidate rows.")
        d2 = [np.inf] * len(starts)
    n_more = n_samples - len(starts)
    if n_more > 0 and not random_tie_break:
        dp.begin(starts, alive_ranked)
        ranks, dd = dp.picks(n_more)
        starts, d2 = starts + ranks.tolist(), d2 + dd.tolist()
    elif n_more > 0:
        count = dp.begin(starts, alive_ranked, want_count=True)
        for p in range(n_more):
            k = int(np.random.choice(count))  # drawn at every pick, also when count == 1 (as np.random.choice(max_indices))
            rank, dd, count = dp.pick_kth(k, want_count=p + 1 < n_more)
            starts.append(rank)
            d2.append(dd)
    return dp.order[starts].tolist(), np.asarray(d2, dtype=np.float64)


def _validate(points, n_samples, initialization):
    """The reference's argument checks, in its order and words (sampling_algorithms.py:60-109)."""
    if n_samples < 1:
        raise ValueError(f"The number of requested samples must be at least 1. Provided: {n_samples=}.")
    if (n_dims := np.ndim(points)) != 2:
        raise ValueError(f"The provided array must be two-dimensional but the given input had {n_dims} dimensions.")
    if (n_points := len(points)) == 0:
        raise ValueError("The provided array must contain at least one row.")
    if points.shape[-1] == 0:
        raise ValueError("The provided input space must be at least one-dimensional.")
    if isinstance(initialization, Collection) and all(isinstance(x, int) for x in initialization):
        if duplicates := {k for k, v in Counter(initialization).items() if v > 1}:
            raise ValueError(
                f"The provided collection of initialization indices must be unique but contains duplicates: {duplicates}")
        if len(initialization) > n_points:
            raise ValueError(
                f"The number of provided initialization indices ({len(initialization)}) cannot be larger than the total number of "
                f"points provided ({n_points}).")
        if problematic_indices := [idx for idx in initialization if not (0 <= idx < n_points)]:
            raise ValueError(
                f"The provided collection of initialization indices must be within the range of available points (0 to "
                f"{n_points - 1}) but contains out-of-bounds indices: {problematic_indices}")
        if len(initialization) == 0:
            raise ValueError("The provided collection of initialization indices is empty.")
    elif initialization not in {"farthest", "random"}:
        raise ValueError(
            f"Unknown initialization type. Expected 'farthest', 'random', or a collection of integers. Provided: {initialization=}")
    if n_samples > n_points:
        raise ValueError(
            f"The number of requested samples ({n_samples}) cannot be larger than the total number of points provided ({n_points}).")


def farthest_point_sampling(points: np.ndarray, n_samples: int = 1, initialization="farthest", random_tie_break: bool = True, *,
                            device: int = 0, return_distances: bool = False):
    """``baybe.utils.sampling_algorithms.farthest_point_sampling`` on the device: the positional indices of the selected points.
    With ``return_distances`` also the minimum squared distance to the selection at which each point was picked (the pair's for both
    points of a "farthest" start, ``inf`` for other start points)."""
    _validate(points, n_samples, initialization)
    values = np.ascontiguousarray(points, dtype=np.float64)
    d = values.shape[1]
    dp = _points_factory(values, np.zeros(d), np.ones(d), device)  # (x - 0) / 1: the points themselves, bit for bit
    idx, d2 = _select(dp, n_samples, initialization, random_tie_break)
    return (idx, d2) if return_distances else idx


_points_factory = DevicePoints


def polytope_samples(bounds, equality_constraints=None, inequality_constraints=None, n: int = 1, n_steps: int | None = None,
                     seed: int | None = None, device: int = 0) -> np.ndarray:
    """Uniform samples [n, dc] of the polytope ``{lo <= x <= hi, sum coeff x[idx] = rhs, sum coeff x[idx] >= rhs}`` in the argument
    format of ``botorch.utils.sampling.get_polytope_samples`` - ``bounds`` [2, dc], ``(indices, coefficients, rhs)`` triples - which
    is what ``SubspaceContinuous.sample_uniform`` asks BoTorch for (baybe/searchspace/continuous.py:544-571).  Instead of one
    sequential hit-and-run chain (10 000 burn-in steps, thinning 32) every sample is the end of its own chain of ``n_steps`` steps
    from the Chebyshev centre, all chains advancing together on the device (``bbh_polytope_sample``); ``n_steps`` defaults to
    ``polytope.default_n_steps(dz)``.  The uniforms are counter-based: the same ``seed`` gives the same rows, and the first rows of
    a larger call.  ``seed=None`` draws one from torch's global generator, as the MC samplers of the recommenders do."""
    from baybe_amd.engine import HipGP, draw_sampler_seed
    from baybe_amd.polytope import Polytope

    if int(n) < 0:
        raise ValueError(f"The number of requested samples must be non-negative. Provided: {n=}.")
    poly = Polytope.from_botorch(bounds, equality_constraints, inequality_constraints)
    gp = HipGP(device)
    try:
        return poly.sample(gp, int(n), n_steps, draw_sampler_seed() if seed is None else int(seed)).cpu().numpy()
    finally:
        gp.close()


def _convert_initialization(value) -> str:
    """``FPSInitialization`` (nonpredictive/sampling.py:77-84) by value or member."""
    name = str(getattr(value, "value", value))
    if name not in ("farthest", "random"):
        raise ValueError(f"'{value}' is not a valid FPSInitialization")
    return name


class HipFPSRecommenderImpl:
    """Behaviour of the farthest-point-sampling recommender on an MI355X.  No fields (see ``baybe_amd.plugin``): they are attached by
    ``attrs.make_class`` - below for the stand-alone class, in ``plugin.make_baybe_fps_recommender`` on top of BayBE's
    ``NonPredictiveRecommender``, whose ``recommend`` then drives ``_recommend_discrete``."""

    __slots__ = ()

    is_available = _availability_property()
    _SHARED_ON_COPY: ClassVar[tuple] = ("_fps_cache",)  # the resident point matrix: shared by copies, read-only

    def __deepcopy__(self, memo):
        from copy import deepcopy

        cls = type(self)
        new = cls.__new__(cls)
        memo[id(self)] = new
        for a in attrs.fields(cls):
            val = getattr(self, a.name)
            object.__setattr__(new, a.name, val if a.name in self._SHARED_ON_COPY else deepcopy(val, memo))
        return new

    def __getstate__(self):
        """Pickling: the device-resident matrix stays behind (it is prepared again from the search space on first use)."""
        return {a.name: (None if a.name in self._SHARED_ON_COPY else getattr(self, a.name)) for a in attrs.fields(type(self))}

    def __setstate__(self, state):
        for k, v in state.items():
            object.__setattr__(self, k, v)

    def _resident_points(self, subspace_discrete):
        """(points, labels): the scaled, ranked comp rep of the WHOLE discrete subspace, resident per search space and keyed on its
        content like the Bayesian recommender's candidate matrix; later calls send only a mask."""
        from baybe_amd.recommenders import _content_hash, _frame_content_hash

        comp_rep = subspace_discrete.comp_rep
        idx = comp_rep.index
        idx_key = (idx.start, idx.stop, idx.step) if isinstance(idx, pd.RangeIndex) else _content_hash(np.asarray(idx))
        key = (comp_rep.shape, tuple(comp_rep.columns), _frame_content_hash(comp_rep), idx_key, self.device)
        if self._fps_cache is None or self._fps_cache[0] != key:
            values = np.ascontiguousarray(comp_rep.to_numpy(dtype=np.float64))
            mean, scale = standard_scaling(values)  # fitted on the entire search space (nonpredictive/sampling.py:152-157)
            self._fps_cache = (key, _points_factory(values, mean, scale, self.device), comp_rep.index)
        return self._fps_cache[1], self._fps_cache[2]

    def _recommend_discrete(self, subspace_discrete, candidates_exp: pd.DataFrame, batch_size: int) -> pd.Index:
        dp, labels = self._resident_points(subspace_discrete)
        alive = None
        if len(candidates_exp) != len(labels) or not candidates_exp.index.equals(labels):
            pos = labels.get_indexer(candidates_exp.index)
            if (pos < 0).any():
                raise KeyError("candidates contain rows that are not part of the discrete subspace")
            alive = np.zeros(len(labels), dtype=bool)
            alive[pos] = True
        rows, _ = _select(dp, batch_size, self.initialization, self.random_tie_break, alive)
        return labels[np.asarray(rows, dtype=np.int64)]

    def __str__(self) -> str:
        return f"{self.__class__.__name__}(initialization={self.initialization!r}, random_tie_break={self.random_tie_break})"


def fps_recommender_fields() -> dict:
    """attrs fields of the recommender: the reference's two (nonpredictive/sampling.py:101-131) plus the device and the cache."""
    return {
        "initialization": field(default="farthest", converter=_convert_initialization),
        "random_tie_break": field(default=attrs.Factory(lambda self: self.initialization != "farthest", takes_self=True),
                                  validator=instance_of(bool), kw_only=True),
        "device": field(default=0, validator=instance_of(int), kw_only=True),
        "_fps_cache": field(default=None, init=False, eq=False, repr=False),
    }


class _StandAloneFPS(HipFPSRecommenderImpl):
    """``NonPredictiveRecommender.recommend`` -> ``PureRecommender.recommend`` for discrete spaces, where BayBE is not importable
    (nonpredictive/base.py:21-58, pure/base.py:248-310)."""

    __slots__ = ()

    def recommend(self, batch_size, searchspace, objective=None, measurements=None, pending_experiments=None) -> pd.DataFrame:
        if pending_experiments is not None:
            raise IncompatibleArgumentError(
                f"Pending experiments were passed to '{self.__class__.__name__}.recommend' but non-predictive recommenders cannot "
                f"use this information. If you want to exclude the pending experiments from the candidate set, adjust the search "
                f"space accordingly.")
        if (measurements is not None) and not measurements.empty:
            warnings.warn(
                f"'recommend' was called with a non-empty set of measurements but '{self.__class__.__name__}' does not utilize any "
                f"training data, meaning that the argument is ignored.", UnusedObjectWarning)
        if objective is not None:
            warnings.warn(
                f"'recommend' was called with a an explicit objective but '{self.__class__.__name__}' does not consider any "
                f"objectives, meaning that the argument is ignored.", UnusedObjectWarning)
        candidates_exp, _ = searchspace.discrete.get_candidates()
        if len(candidates_exp) < batch_size:
            raise NotEnoughPointsLeftError(
                f"Using the current settings, there are fewer than {batch_size} possible data points left to recommend.")
        idxs = self._recommend_discrete(searchspace.discrete, candidates_exp, batch_size)
        return searchspace.discrete.exp_rep.loc[idxs, :]


HipFPSRecommender = attrs.make_class("HipFPSRecommender", fps_recommender_fields(), bases=(_StandAloneFPS,), slots=False)
HipFPSRecommender.__doc__ = "Initial recommender selecting candidates by farthest point sampling on an MI355X (stand-alone)."
HipFPSRecommender.__module__ = __name__
HipFPSRecommender.compatibility = "DISCRETE"
