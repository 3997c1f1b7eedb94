"""Plain numpy / scipy statements of what ``baybe_amd/csrc/bbh_polytope.hip`` computes, independent of the product:

(a) ``sample_oracle``   the hit-and-run sampler in ``uint64`` / ``float64`` with the same counter function and operation order;
(b) ``project_exact``   the Euclidean projection by enumeration of the active sets (dc <= 4, at most 12 rows, box included);
(c) ``kkt_residual``    how far ``x - p`` is from the cone of the active normals at ``x``, for any size.

Sets are given as ``(lo, hi, E, e, G, g)``: ``lo <= c <= hi``, ``E c = e``, ``G c >= g``.
"""

from __future__ import annotations

import itertools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


# ---- (a) the sampler ---------------------------------------------------------------------------------------------------------------
def mix64(z):
    """SplitMix64's finaliser on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def chain_keys(seed: int, chains) -> np.ndarray:
    with np.errstate(over="ignore"):
        s = mix64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) + GOLDEN)
        return mix64(s + GOLDEN * (np.asarray(chains, dtype=np.uint64) + np.uint64(1)))


def uniforms(keys: np.ndarray, step: int, draw: int) -> np.ndarray:
    """u = (h >> 11) 2^-53 of h = mix(key + G (64 step + draw + 1))."""
    with np.errstate(over="ignore"):
        h = mix64(keys + GOLDEN * np.uint64(64 * step + draw + 1))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0**-53


def reduce_set(lo, hi, E, e, G, g):
    """(c0, Z) of the set, independently of the product: an orthonormal basis of null(E) and the Chebyshev centre of the reduced set."""
    from scipy.optimize import linprog

    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    dc = len(lo)
    E, G = np.asarray(E, float).reshape(-1, dc), np.asarray(G, float).reshape(-1, dc)
    e, g = np.asarray(e, float).reshape(-1), np.asarray(g, float).reshape(-1)
    if len(E):
        Z = np.linalg.svd(E, full_matrices=True)[2][len(E):].T
        cp = np.linalg.lstsq(E, e, rcond=None)[0]
    else:
        Z, cp = np.eye(dc), np.zeros(dc)
    dz = Z.shape[1]
    A = np.vstack([Z, -Z, G @ Z])
    b = np.concatenate([lo - cp, cp - hi, g - G @ cp])
    nrm = np.linalg.norm(A, axis=1)
    keep = nrm > 1e-13
    cost = np.zeros(dz + 1)
    cost[-1] = -1.0
    res = linprog(cost, A_ub=np.hstack([-A[keep], nrm[keep, None]]), b_ub=-b[keep], bounds=[(None, None)] * dz + [(0, None)], method="highs")
    assert res.status == 0 and res.x[-1] > 0
    return cp + Z @ res.x[:dz], Z


def sample_oracle(c0, Z, lo, hi, G, g, R: int, T: int, seed: int, first: int = 0) -> np.ndarray:
    """The chains ``first .. first + R`` of ``bbh_polytope_sample``: [R, dc].  Every chain starts at c0 (y = 0) and takes T steps in
    c = c0 + Z y; sums run over the columns ascending from 0.0, every product and sum rounded (numpy contracts nothing)."""
    c0, lo, hi = (np.asarray(v, dtype=np.float64) for v in (c0, lo, hi))
    Z = np.asarray(Z, dtype=np.float64)
    dc, dz = Z.shape
    G = np.asarray(G, dtype=np.float64).reshape(-1, dc)
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    GZ, bl, bu, bg = G @ Z, lo - c0, hi - c0, g - G @ c0
    return sample_oracle_reduced(Z, GZ, c0, lo, hi, bl, bu, bg, R, T, seed, first)


def sample_oracle_reduced(Z, GZ, c0, lo, hi, bl, bu, bg, R: int, T: int, seed: int, first: int = 0) -> np.ndarray:
    """As ``sample_oracle`` on the arrays the kernel is handed (so that no matrix product of the set-up is done twice)."""
    dc, dz = Z.shape
    rows = np.vstack([Z, GZ.reshape(-1, dz)])  # [dc + mi, dz]
    keys = chain_keys(seed, np.arange(first, first + R))
    y = np.zeros((R, dz))
    with np.errstate(divide="ignore", invalid="ignore"):
        for step in range(T):
            d = np.stack([uniforms(keys, step, j) - 0.5 for j in range(dz)], axis=1)
            up = uniforms(keys, step, dz)
            w = np.zeros((R, rows.shape[0]))
            v = np.zeros((R, rows.shape[0]))
            for j in range(dz):
                w = w + rows[None, :, j] * y[:, j, None]
                v = v + rows[None, :, j] * d[:, j, None]
            wb, vb = w[:, :dc], v[:, :dc]
            sl, su = wb - bl, bu - wb
            pos, neg = vb > 0, vb < 0
            lo_c = np.where(pos, -sl / vb, np.where(neg, su / vb, -np.inf))
            hi_c = np.where(pos, su / vb, np.where(neg, -sl / vb, np.inf))
            tlo, thi = lo_c.max(axis=1), hi_c.min(axis=1)
            if rows.shape[0] > dc:
                s, vg = w[:, dc:] - bg, v[:, dc:]
                tlo = np.maximum(tlo, np.where(vg > 0, -s / vg, -np.inf).max(axis=1))
                thi = np.minimum(thi, np.where(vg < 0, -s / vg, np.inf).min(axis=1))
            tlo, thi = np.minimum(tlo, 0.0), np.maximum(thi, 0.0)
            fin = np.isfinite(tlo) & np.isfinite(thi)
            t = np.where(fin, np.where(fin, tlo, 0.0) + up * (np.where(fin, thi, 0.0) - np.where(fin, tlo, 0.0)), 0.0)
            y = y + t[:, None] * d
    acc = np.zeros((R, dc))
    for j in range(dz):
        acc = acc + Z[None, :, j] * y[:, j, None]
    return np.clip(c0 + acc, lo, hi)


def simplex_moments(dc: int):
    """(mean, variance, variance of x^2-centred estimator inputs) of a coordinate of the uniform distribution on the simplex
    sum c = 1, c >= 0 (Beta(1, dc - 1)): mean 1/dc, variance (dc-1)/(dc^2 (dc+1)), and the fourth central moment."""
    raw = [1.0]
    for k in range(1, 5):  # E x^k = k! / (dc (dc+1) ... (dc+k-1))
        raw.append(raw[-1] * k / (dc + k - 1))
    m1, m2, m3, m4 = raw[1:]
    var = m2 - m1 * m1
    mu4 = m4 - 4 * m1 * m3 + 6 * m1 * m1 * m2 - 3 * m1**4
    return m1, var, mu4


def moment_z_scores(X: np.ndarray, dc: int):
    """Per coordinate: (sample mean - 1/dc) and (sample variance - analytic) in standard errors of n independent draws."""
    n = len(X)
    m1, var, mu4 = simplex_moments(dc)
    z_mean = (X.mean(axis=0) - m1) / np.sqrt(var / n)
    z_var = (X.var(axis=0, ddof=1) - var) / np.sqrt((mu4 - var * var * (n - 3) / (n - 1)) / n)
    return z_mean, z_var


# ---- (b) the exact projection --------------------------------------------------------------------------------------------------------
def project_exact(p, lo, hi, E, e, G, g):
    """The projection of p onto the set by enumeration: every subset of the inequality and box rows as the active set, the
    equality-constrained projection of each (least-squares multipliers, so dependent active rows are fine), the feasible candidate
    with sign-correct multipliers that is closest to p.  dc <= 4 and at most 12 rows, box included."""
    p, lo, hi = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (p, lo, hi))
    dc = len(p)
    E = np.asarray(E, dtype=np.float64).reshape(-1, dc)
    G = np.asarray(G, dtype=np.float64).reshape(-1, dc)
    e, g = np.asarray(e, dtype=np.float64).reshape(-1), np.asarray(g, dtype=np.float64).reshape(-1)
    A = np.vstack([G, np.eye(dc), -np.eye(dc)])  # A x >= b
    b = np.concatenate([g, lo, -hi])
    assert dc <= 4 and len(b) <= 12, "enumeration oracle: dc <= 4, at most 12 rows"
    me = len(E)
    scale = max(1.0, float(np.abs(p).max()))
    best, best_d = None, np.inf
    for n_act in range(0, len(b) + 1):
        for act in itertools.combinations(range(len(b)), n_act):
            N = np.vstack([E, A[list(act)]])
            rhs = np.concatenate([e, b[list(act)]])
            if len(N):
                lam, *_ = np.linalg.lstsq(N @ N.T, rhs - N @ p, rcond=1e-13)
                x = p + N.T @ lam
                if np.abs(N @ x - rhs).max() > 1e-11 * scale:
                    continue  # inconsistent active set
                if (lam[me:] < -1e-11 * scale).any():
                    continue
            else:
                x = p.copy()
            if (A @ x - b < -1e-11 * scale).any() or (len(E) and np.abs(E @ x - e).max() > 1e-11 * scale):
                continue
            d = float(np.linalg.norm(x - p))
            if d < best_d:
                best, best_d = x, d
    assert best is not None, "empty set"
    return best


# ---- (c) the KKT residual --------------------------------------------------------------------------------------------------------------
def kkt_residual(p, x, lo, hi, E, e, G, g, act_tol: float = 1e-9) -> float:
    """x is the projection of p iff x is feasible and x - p = sum lambda_i n_i over the inward normals n_i of the active inequality
    and box rows (lambda >= 0) and +- the equality rows.  Returns the ``scipy.optimize.nnls`` residual of that fit relative to
    max(1, |p - x|).  Rows within ``act_tol`` (relative to their terms) of equality count as active."""
    from scipy.optimize import nnls

    p, x, lo, hi = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (p, x, lo, hi))
    dc = len(p)
    E = np.asarray(E, dtype=np.float64).reshape(-1, dc)
    G = np.asarray(G, dtype=np.float64).reshape(-1, dc)
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    cols = [r for r in E] + [-r for r in E]
    slack = G @ x - g
    sabs = np.abs(G * x).sum(axis=1) + np.abs(g)
    cols += [G[i] for i in range(len(G)) if slack[i] <= act_tol * max(sabs[i], 1e-300)]
    span = np.maximum(hi - lo, 1e-300)
    for k in range(dc):
        if x[k] - lo[k] <= act_tol * span[k]:
            cols.append(np.eye(dc)[k])
        if hi[k] - x[k] <= act_tol * span[k]:
            cols.append(-np.eye(dc)[k])
    r = x - p
    if not cols:
        return float(np.linalg.norm(r) / max(1.0, np.linalg.norm(r)))
    _, rn = nnls(np.array(cols).T, r, maxiter=50 * (len(cols) + dc))
    return float(rn / max(1.0, np.linalg.norm(r)))


def feasibility_ratio(X, lo, hi, E, e, G, g, C: float) -> np.ndarray:
    """Per row of X: the worst of |E x - e|_i and (g - G x)_i^+ over the bound C (dc + M) eps S_abs,i, S_abs,i = sum_k |row_ik x_k| +
    |rhs_i|, M = 2 dc + mi; inf for a row that leaves [lo, hi] by a single bit."""
    X = np.asarray(X, dtype=np.float64)
    dc = X.shape[1]
    E, G = np.asarray(E, float).reshape(-1, dc), np.asarray(G, float).reshape(-1, dc)
    e, g = np.asarray(e, float).reshape(-1), np.asarray(g, float).reshape(-1)
    worst = np.where(((X < lo) | (X > hi)).any(axis=1), np.inf, 0.0)
    factor = C * (dc + 2 * dc + len(g)) * EPS
    for rows, rhs, two_sided in ((E, e, True), (G, g, False)):
        for r, b in zip(rows, rhs):
            terms = X * r
            res = terms.sum(axis=1) - b
            viol = np.abs(res) if two_sided else np.maximum(-res, 0.0)
            bound = factor * (np.abs(terms).sum(axis=1) + abs(b))
            worst = np.maximum(worst, np.where(viol > 0, viol / np.maximum(bound, 1e-300), 0.0))
    return worst


# ---- fixtures shared by the CPU and the GPU tests ------------------------------------------------------------------------------------------
def simplex(dc: int):
    """sum c = 1 on [0, 1]^dc."""
    return np.zeros(dc), np.ones(dc), np.ones((1, dc)), np.ones(1), np.zeros((0, dc)), np.zeros(0)


def random_set(dc: int, me: int, mi: int, seed: int):
    """A set with ``me`` independent equalities and ``mi`` inequalities on a box that is not the unit box, all of them passing at
    distance >= 0.05 of an interior point (so the set has interior), rows of mixed sign and scale."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-1.0, 0.0, dc)
    hi = lo + rng.uniform(0.5, 2.0, dc)
    centre = lo + (hi - lo) * rng.uniform(0.3, 0.7, dc)
    E = rng.normal(size=(me, dc)) * rng.uniform(0.5, 3.0, (me, 1))
    e = E @ centre
    G = rng.normal(size=(mi, dc)) * rng.uniform(0.5, 3.0, (mi, 1))
    g = G @ centre - rng.uniform(0.05, 0.3, mi) * np.linalg.norm(G, axis=1)
    return lo, hi, E, e, G, g
