"""TEST INFRASTRUCTURE - qExpectedHypervolumeImprovement / qLogExpectedHypervolumeImprovement restated in numpy for
tests/test_ehvi_cpu.py and tests/test_ehvi_gpu.py.  Deliberately NOT shared with ``baybe_amd/ehvi.py``.

[UPSTREAM] PARITY UNPINNED, as ``oracle/nehvi_oracle.py``: BoTorch is not importable here, so its implementation
(botorch/acquisition/multi_objective/monte_carlo.py ``qExpectedHypervolumeImprovement``, .../logei.py
``qLogExpectedHypervolumeImprovement``, .../base.py ``MultiObjectiveMCAcquisitionFunction``, utils/safe_math.py) is restated from
memory, and the following could not be checked against the source: the default of ``alpha`` (0 for up to 4 objectives), the order in
which the log form reduces (below), the clamp of the cell upper bounds at 1e10, and the sample count 128.
Reference call sites: ``baybe/acquisition/acqfs.py:429-464`` (the two classes, ``alpha``), ``baybe/acquisition/_builder.py:286-299``
(``partitioning`` from ``_posterior_mean_comp``), ``baybe/acquisition/utils.py:26-84`` (``make_partitioning``).

One fixed cell list (l_c, u_c), c < C (u may be +inf), from the box decomposition of the models' oriented posterior means at all
measurement rows.  ``optimize_acqf_discrete`` concatenates earlier picks and pending experiments to every candidate, so a candidate
scores the joint batch [x_i ; pending] of q' points; the m targets are independent, the q' points of one target jointly Gaussian,
base samples [S, q', m].  With y[r, j] the oriented draw of point r, target j in sample s:

  qEHVI     (1/S) sum_s sum_c sum_{A != {}} (-1)^(|A|+1) prod_j max(0, min(min_{r in A} y[r, j], u_c[j]) - l_c[j])
  qLogEHVI  li[c, r, j] = log_fatplus(y[r, j] - l_c[j]; 1e-6);  per subset A: fatmin_{r in A} li (= -fatmax(-.), tau 1e-2, alpha 2; one
            member: the value itself), fatmin2 of that against log(min(u_c[j], 1e10) - l_c[j]), summed over j;  logsumexp over the
            subsets of one size;  the sizes accumulated by logaddexp into an odd and an even slot;  per cell logdiffexp(odd, even);
            logsumexp over the cells;  logmeanexp over the samples.

Both are written with ``itertools.combinations`` over the points and vectorised over rows, samples and cells.  ``dtype`` runs the whole
evaluation in another precision (``np.longdouble``: the guard of the fixtures)."""

from __future__ import annotations

from itertools import combinations

import numpy as np

from oracle import gp_oracle as go
from oracle import nehvi_oracle as no

TAU_RELU, TAU_MAX, UPPER_CLAMP = no.TAU_RELU, no.TAU_MAX, no.UPPER_CLAMP


def log_fatplus(x, tau=TAU_RELU):
    """log(tau (softplus(x / tau) + 0.1 / (1 + (x / tau)^2))), torch's softplus threshold 20, in the precision of x."""
    t = x / tau
    sp = np.where(t > 20.0, t, np.log1p(np.exp(np.minimum(t, 20.0))))
    return np.log(x.dtype.type(tau)) + np.log(sp + 0.1 / (1.0 + t * t))


def fatmin(x, axis, tau=TAU_MAX, alpha=2.0):
    """-fatmax(-x) along ``axis``."""
    mn = x.min(axis=axis, keepdims=True)
    s = ((alpha / (alpha + (x - mn) / tau)) ** alpha).sum(axis=axis)
    return np.squeeze(mn, axis=axis) - tau * np.log(s)


def fatmin2(a, b, tau=TAU_MAX, alpha=2.0):
    return np.minimum(a, b) - tau * np.log1p((alpha / (alpha + np.abs(a - b) / tau)) ** alpha)


def logsumexp(x, axis):
    M = x.max(axis=axis, keepdims=True)
    M = np.where(np.isfinite(M), M, 0.0)
    return np.squeeze(M, axis=axis) + np.log(np.exp(x - M).sum(axis=axis))


def logdiffexp(a, b):
    """log(e^a - e^b) = a + log1mexp(b - a) [UPSTREAM safe_math.logdiffexp]."""
    x = b - a
    with np.errstate(all="ignore"):  # (b > a: NaN, as upstream)
        return a + np.where(x > -np.log(2.0), np.log(-np.expm1(x)), np.log1p(-np.exp(x)))


def qehvi_samples(Y, lo, up):
    """Y [..., q, m] oriented draws -> [...] hypervolume improvement of the q points against the cells (inclusion-exclusion)."""
    q = Y.shape[-2]
    a = np.minimum(Y[..., None, :, :], up[:, None, :]) - lo[:, None, :]  # [..., C, q, m]
    total = np.zeros(a.shape[:-2], dtype=Y.dtype)
    for i in range(1, q + 1):
        for A in combinations(range(q), i):
            side = np.maximum(a[..., list(A), :].min(axis=-2), 0.0)
            total = total + (-1.0) ** (i + 1) * side.prod(axis=-1)
    return total.sum(axis=-1)


def qlogehvi_samples(Y, lo, up):
    """Y [..., q, m] -> [...] smoothed log hypervolume improvement per sample (steps 1 - 8 of the module docstring)."""
    q = Y.shape[-2]
    li = log_fatplus(Y[..., None, :, :] - lo[:, None, :])  # [..., C, q, m]
    with np.errstate(divide="ignore"):
        ll = np.log(np.minimum(up, UPPER_CLAMP) - lo)  # [C, m]
    slots = {1: None, 0: None}
    for i in range(1, q + 1):
        terms = []
        for A in combinations(range(q), i):
            fm = li[..., A[0], :] if i == 1 else fatmin(li[..., list(A), :], axis=-2)
            terms.append(fatmin2(fm, ll).sum(axis=-1))
        lse = logsumexp(np.stack(terms, axis=-1), axis=-1)
        slots[i % 2] = lse if slots[i % 2] is None else np.logaddexp(slots[i % 2], lse)
    with np.errstate(all="ignore"):
        cell = slots[1] if slots[0] is None else logdiffexp(slots[1], slots[0])
    return logsumexp(cell, axis=-1)


def reduce_samples(log: bool, Y, lo, up):
    """Y [N, S, q, m] -> [N]."""
    if not log:
        return qehvi_samples(Y, lo, up).mean(axis=-1)
    v = qlogehvi_samples(Y, lo, up)
    return logsumexp(v, axis=-1) - np.log(Y.dtype.type(Y.shape[1]))


def scores_from_factors(log: bool, means, L, z, lo, up, signs=None, dtype=np.float64):
    """means [m, N, q], L [m, N, q, q] lower factors, z [S, q, m], cells [C, m] -> [N] (NaN where a factor is NaN).  ``signs``: the
    draws of target j are multiplied by signs[j] (None: the statistics are oriented already)."""
    m = len(means)
    means, L, z, lo, up = (np.asarray(a, dtype=dtype) for a in (means, L, z, lo, up))
    sg = np.ones(m, dtype=dtype) if signs is None else np.asarray(signs, dtype=dtype)
    with np.errstate(all="ignore"):
        Y = np.stack([sg[j] * (means[j][:, None, :] + np.einsum("sc,nrc->nsr", z[:, :, j], L[j])) for j in range(m)], axis=-1)
        return reduce_samples(log, Y, lo, up)  # [N, S, q, m] -> [N]


def q1_scores(log: bool, mu, var, z, lo, up, dtype=np.float64):
    """mu / var [m, N], z [S, m]: 1 x 1 factors with psd_safe_cholesky's jitter."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    sd = np.stack([go._safe_sqrt_var(v) for v in var])
    return scores_from_factors(log, mu[:, :, None], sd[:, :, None, None], np.asarray(z, dtype=np.float64)[:, None, :], lo, up, dtype=dtype)


def sigma(var, cross, cpp):
    """[N, q, q] joint covariances of one target."""
    N, p = cross.shape
    Sig = np.empty((N, p + 1, p + 1))
    Sig[:, 0, 0], Sig[:, 0, 1:], Sig[:, 1:, 0], Sig[:, 1:, 1:] = var, cross, cross, cpp
    return Sig


def joint_means(mu, mp):
    return np.stack([np.concatenate([a[:, None], np.broadcast_to(b, (len(a), len(b)))], axis=1) for a, b in zip(mu, mp)])


def lapack_factors(Sig):
    """``_safe_cholesky`` of every matrix of the stack [N, q, q]; NaN where it raises."""
    import scipy.linalg as sla

    out = np.full_like(Sig, np.nan)
    for i, A in enumerate(Sig):
        try:
            out[i] = go._safe_cholesky(A)
        except sla.LinAlgError:
            pass
    return out


def joint_scores(log: bool, mu, var, cross, mp, cpp, z, lo, up, signs=None, alive=None):
    """mu / var [m, N], cross [m, N, p], mp [m, p], cpp [m, p, p], z [S, p + 1, m] -> [N]: -inf for masked rows, NaN where a
    target's covariance does not factor."""
    L = np.stack([lapack_factors(sigma(var[j], cross[j], cpp[j])) for j in range(len(mu))])
    out = scores_from_factors(log, joint_means(mu, mp), L, z, lo, up, signs)
    if alive is not None:
        out = np.where(np.asarray(alive).astype(bool), out, -np.inf)
    return out


# ---- on fitted oracle models, one per target (end-to-end comparisons) ---------------------------------------------------------------
def base_samples(S, q, m, seed):
    return go.sobol_normal_base_samples(S, q * m, seed).reshape(S, q, m)


def model_cells(models, signs, X_all, ref):
    """The partitioning of the models' oriented posterior means at ALL measurement rows."""
    mu = np.stack([mod.posterior(X_all)[0] for mod in models], axis=-1) * np.asarray(signs)[None, :]
    return no.nondominated_cells(mu, ref)


def model_scores(log: bool, models, signs, X, pend, z, lo, up):
    """Scores of the t-batches [x_i ; pend] under the oracle models' joint posteriors; z [S, q, m]."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    N = len(X)
    if pend is None or len(pend) == 0:
        mv = [mod.posterior(X) for mod in models]
        mu, var = np.stack([a for a, _ in mv]), np.stack([b for _, b in mv])
        sd = np.stack([go._safe_sqrt_var(v) for v in var])
        return scores_from_factors(log, mu[:, :, None], sd[:, :, None, None], np.asarray(z), lo, up, signs)
    mu, var, cross, mp, cpp = [], [], [], [], []
    for mod in models:
        a, cov = mod.posterior_joint(np.vstack([X, pend]))
        mu.append(a[:N]), var.append(np.diag(cov)[:N].copy()), cross.append(cov[:N, N:]), mp.append(a[N:]), cpp.append(cov[N:, N:])
    return joint_scores(log, np.stack(mu), np.stack(var), np.stack(cross), np.stack(mp), np.stack(cpp), z, lo, up, signs)


def greedy(log: bool, models, signs, X, q, seed, X_all, ref, S=128, pending=None):
    """Sequential greedy of ``optimize_acqf_discrete`` (first index on ties, picks leave the candidate set):
    (indices, values, gaps) - gaps[k]: best minus second-best score of step k."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    lo, up = model_cells(models, signs, X_all, ref)
    base = np.zeros((0, X.shape[1])) if pending is None else np.atleast_2d(pending)
    live = np.ones(len(X), dtype=bool)
    idx, vals, gaps = [], [], []
    for _ in range(q):
        pend = np.vstack([base, X[idx]]) if idx else base
        z = base_samples(S, 1 + len(pend), len(models), seed)
        s = np.where(live, model_scores(log, models, signs, X, pend, z, lo, up), -np.inf)
        i = int(np.argmax(s))
        top = np.sort(s[live])[-2:]
        idx.append(i), vals.append(float(s[i])), gaps.append(float(top[1] - top[0]))
        live[i] = False
    return idx, vals, gaps
