"""Numpy restatement of the forest surrogate's device side (TEST INFRASTRUCTURE; imports nothing of ``baybe_amd``).

What the reference does (``baybe/surrogates/random_forest.py``): ``predictor.predict(candidates)`` per tree into an ``[T, N]`` matrix,
an ``EnsemblePosterior`` over it, and BoTorch's ``IndexSampler``: MC sample ``s`` IS ensemble member ``idx_s``.  Restated here:
  * ``traverse``: a tree's prediction - the row cast to float32, left iff ``float64(x32[feature]) <= threshold``;
  * ``moments``: mean and unbiased variance over the trees (two passes, ``ddof=1``, zero for one tree);
  * ``scores``: the MC acquisition values, gathering ``P[idx_s]`` literally for every one of the S samples and applying
    ``log_fatplus`` / ``fatmax`` / ``logmeanexp`` / ``_mc_utility`` of ``oracle/gp_oracle.py`` to the t-batches [x_i ; pending];
  * ``scores_from_counts``: the same from ``counts[t] = #{s : idx_s = t}`` - the form the device evaluates;
  * ``greedy``: sequential greedy selection, first-index argmax, per step the margin to the best row that does not tie with the winner, judged in extended precision.
"""

from __future__ import annotations

import math

import numpy as np

from oracle import gp_oracle as go


def traverse(packed: dict, X: np.ndarray) -> np.ndarray:
    """``P [T, N]``: ``estimators_[t].predict(X)`` restated on the packed arrays."""
    X32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    off = packed["offsets"]
    T, N = len(off) - 1, len(X32)
    P = np.empty((T, N))
    rows = np.arange(N)
    for t in range(T):
        sl = slice(off[t], off[t + 1])
        left, right, feat = packed["children_left"][sl], packed["children_right"][sl], packed["feature"][sl]
        thr, val = packed["threshold"][sl], packed["value"][sl]
        node = np.zeros(N, dtype=np.int64)
        for _ in range(len(left)):
            inner = left[node] >= 0
            if not inner.any():
                break
            x = X32[rows, np.where(inner, feat[node], 0)].astype(np.float64)
            go_left = x <= thr[node]
            node = np.where(inner, np.where(go_left, left[node], right[node]), node)
        P[t] = val[node]
    return P


def moments(P: np.ndarray):
    """(mean [N], unbiased variance [N]) over the trees; the variance is exactly 0 for one tree."""
    T = P.shape[0]
    mean = P.sum(axis=0) / T
    if T == 1:
        return mean, np.zeros_like(mean)
    return mean, ((P - mean[None, :]) ** 2).sum(axis=0) / (T - 1)


def best_f(P_train: np.ndarray, sign: float) -> float:
    """max_i sign * mean_t P_t(x_i) over the training inputs (acquisition/_builder.py:141-161)."""
    return float((sign * moments(P_train)[0]).max())


def _batches(Px: np.ndarray, Ppend: np.ndarray | None, sign: float) -> np.ndarray:
    """obj [T, N, 1 + k]: per tree the t-batch [x_i ; pending], the candidate first."""
    T, N = Px.shape
    k = 0 if Ppend is None else Ppend.shape[1]
    obj = np.empty((T, N, 1 + k))
    obj[:, :, 0] = sign * Px
    if k:
        obj[:, :, 1:] = sign * Ppend[:, None, :]
    return obj


def _log_fatplus_wide(x):
    """``gp_oracle.log_fatplus`` restated for extended precision (the oracle's own casts its argument to float64)."""
    t = x / type(x.flat[0])(go.TAU_RELU)
    with np.errstate(over="ignore"):
        sp = np.where(t > 20, t, np.log1p(np.exp(np.minimum(t, 20))))
    return np.log(type(x.flat[0])(go.TAU_RELU)) + np.log(sp + type(x.flat[0])(go.FAT_ALPHA_PLUS) / (1 + t * t))


def scores(kind: str, Px: np.ndarray, Ppend, idx: np.ndarray, best: float, sign: float = 1.0, beta: float = 0.2, wide: bool = False):
    """Acquisition values [N]: sample s reads tree idx[s]; all S samples are gathered and reduced as gp_oracle.mc_acq_joint does.
    ``wide``: the same arithmetic in ``np.longdouble`` (64-bit mantissa on x86) - what ``greedy`` judges near-ties with."""
    samples = _batches(Px, Ppend, sign)[np.asarray(idx)]  # [S, N, 1 + k]
    if wide:
        samples = samples.astype(np.longdouble)
    if kind == "qLogEI":
        li = _log_fatplus_wide(samples - best) if wide else go.log_fatplus(samples - best)
        return go.logmeanexp(go.fatmax(li, axis=-1), axis=0)
    with np.errstate(over="ignore"):  # (qPI's sigmoid at 1e3 (obj - best_f): exp overflows to inf, the utility is the exact 0)
        return go._mc_utility(kind, samples, best, beta).max(axis=-1).mean(axis=0)


def scores_from_counts(kind: str, Px, Ppend, counts: np.ndarray, best: float, sign: float = 1.0, beta: float = 0.2) -> np.ndarray:
    """The same values from the member counts: log sum_t counts[t] exp(v_t - M) + M - log S, resp. the count-weighted mean."""
    counts = np.asarray(counts, dtype=np.float64)
    S = counts.sum()
    used = counts > 0
    obj = _batches(Px, Ppend, sign)[used]  # [T', N, 1 + k]
    w = counts[used][:, None]
    if kind == "qLogEI":
        v = go.fatmax(go.log_fatplus(obj - best), axis=-1)  # [T', N]
        M = v.max(axis=0)
        return np.log((w * np.exp(v - M[None, :])).sum(axis=0)) + M - math.log(S)
    if kind in ("qUCB", "qPSTD"):
        m = (w[:, :, None] * obj).sum(axis=0, keepdims=True) / S
        cu = math.sqrt((beta if kind == "qUCB" else 1.0) * math.pi / 2.0)
        util = (m if kind == "qUCB" else 0.0) + cu * np.abs(obj - m)
    else:
        with np.errstate(over="ignore"):
            util = go._mc_utility(kind, obj, best, beta)
    return (w * util.max(axis=-1)).sum(axis=0) / S


def greedy(kind: str, P: np.ndarray, idx: np.ndarray, best: float, sign: float, batch_size: int, Ppend=None, alive=None,
           beta: float = 0.2):
    """Sequential greedy batch over the candidates whose per-tree predictions are ``P [T, N]``: each step scores [x_i ; pending],
    takes the first index of the maximum among the live rows, appends the pick's column to the pending block and masks the pick.
    Returns (indices, values, margins): margins[j] = the winner's score minus the best score among the live rows that do not tie
    with it, both in extended precision (inf if every live row ties).  Rows tie when their extended-precision scores are equal:
    twins of the winner, rows beaten by the same pending point, rows without any improvement - ties of the function itself, which
    every summation order reproduces.  Two rows whose float64 scores merely ROUND to the same number differ in extended precision
    and give a margin near 0: another summation order could rank them either way, so a fixture must not contain them."""
    alive = np.ones(P.shape[1], dtype=bool) if alive is None else np.asarray(alive, dtype=bool).copy()
    pend = None if Ppend is None or Ppend.shape[1] == 0 else np.array(Ppend)
    picks, values, margins = [], [], []
    for _ in range(batch_size):
        s = np.where(alive, scores(kind, P, pend, idx, best, sign, beta), -np.inf)
        i = int(np.argmax(s))
        w = scores(kind, P, pend, idx, best, sign, beta, wide=True)
        others = w[alive & (w != w[i])]
        margins.append(float(w[i] - others.max()) if others.size else math.inf)
        picks.append(i), values.append(float(s[i]))
        col = P[:, i:i + 1]
        pend = col.copy() if pend is None else np.concatenate([pend, col], axis=1)
        alive[i] = False
    return picks, values, margins
