"""TEST INFRASTRUCTURE - qLogNParEGO and plain qNEHVI restated on the frozen oracle (``oracle/nehvi_oracle.py``).

qLogNParEGO [UPSTREAM botorch.acquisition.multi_objective.parego.qLogNParEGO] is qLogNoisyExpectedImprovement under an augmented
Chebyshev scalarisation of the oriented targets.  ``NEHVIOracle(models, signs, X_b, [-1e9] * m, z)`` holds both halves of the joint
draw, as for ``tests/_nei_reference.py``: ``obj_b`` [S, nb, m] are the oriented baseline samples and ``candidate_samples(x) * signs``
the candidate's draw through the cached baseline factor.

    Y      = oriented posterior means of the m targets at ALL baseline rows (before pruning)
    bounds   lo_o = min_b Y, hi_o = max_b Y; one row: hi = lo + 1; a zero range counts as 1                      [UPSTREAM]
    g(y)   = -(max_o t_o + 0.05 sum_o t_o),  t_o = w_o (hi_o - y_o) / (hi_o - lo_o)       [UPSTREAM get_chebyshev_scalarization]
    best_s = max_b g(obj_b[s, b, :]),  u_s = g(f_s) - best_s,  score = logmeanexp_s log_fatplus(u_s; 1e-6)
    weights  given, or ``sample_simplex``: m - 1 ``torch.rand`` doubles, sorted; differences of [0, ..., 1]      [UPSTREAM]

Plain qNEHVI: ``mean_s hvi_from_cells(f_s, cells_s)`` with qLogNEHVI's per-sample cells."""

import numpy as np

from oracle import gp_oracle as go
from oracle import nehvi_oracle as no

PRUNE_SAMPLES = 2048
ALPHA = 0.05


def base_samples(S, nb, m, seed):
    """[S, nb + 1, m]: one scrambled-Sobol draw of dimension (nb + 1) m, point-major, the candidate's row last."""
    return no.sobol_normal_base_samples_nd(S, nb + 1, m, seed)


def sample_simplex(m):
    """Weights drawn from torch's global generator."""
    import torch

    cuts = np.sort(torch.rand(m - 1, dtype=torch.float64).numpy())
    return np.diff(np.r_[0.0, cuts, 1.0])


def bounds(models, signs, Xb_all):
    """(lo [m], hi [m]) from the oriented posterior means at every baseline row."""
    Y = np.stack([s * mod.posterior(np.atleast_2d(Xb_all))[0] for mod, s in zip(models, signs)], axis=1)
    lo, hi = Y.min(0), Y.max(0)
    if len(Y) == 1:
        hi = lo + 1.0
    return lo, hi


def scalarize(y, w, lo, hi):
    """g over the last axis of y (oriented values)."""
    rng = np.where(hi - lo == 0.0, 1.0, hi - lo)
    t = np.asarray(w) * (hi - y) / rng
    return -(t.max(-1) + ALPHA * t.sum(-1))


def scores(models, signs, Xb, z, X, w, lo, hi):
    """(scores [len(X)], best_s [S], u [len(X), S]) of the q = 1 t-batches X against the baseline Xb (lo / hi: ``bounds`` of the
    acquisition function's whole baseline)."""
    signs = np.asarray(signs, dtype=np.float64)
    orc = no.NEHVIOracle(models, signs, Xb, [-1e9] * len(models), z)
    best = scalarize(orc.obj_b, w, lo, hi).max(1)
    u = np.array([scalarize(orc.candidate_samples(x) * signs[None, :], w, lo, hi) - best for x in np.atleast_2d(X)])
    val = np.array([no.logmeanexp_with_neginf(go.log_fatplus(ui, no.TAU_RELU)) for ui in u])
    return val, best, u


def prune(models, signs, Xb, seed, w, lo, hi):
    """``prune_inferior_points`` under the scalarisation: indices of the baseline rows that are the first-index argmax of g in at
    least one of 2048 joint draws (ascending), and the smallest gap between a sample's best and second-best value.  The draw has the
    layout of qLogNEHVI's pruning draw (``no.prune_baseline``)."""
    Xb = np.atleast_2d(Xb)
    nb, m = len(Xb), len(models)
    z = no.sobol_normal_base_samples_nd(PRUNE_SAMPLES, nb, m, seed)
    F = np.empty((PRUNE_SAMPLES, nb, m))
    for o, mod in enumerate(models):
        mu, cov = mod.posterior_joint(Xb)
        F[:, :, o] = (mu[None, :] + z[:, :, o] @ go._safe_cholesky(cov).T) * signs[o]
    G = scalarize(F, w, lo, hi)
    top2 = np.sort(G, axis=1)[:, -2:]
    return np.unique(G.argmax(1)), float((top2[:, 1] - top2[:, 0]).min()) if nb > 1 else np.inf


def greedy(models, signs, Xb, X, q, S, seed, w, lo, hi, X_pending=None, alive=None):
    """Sequential greedy with picks and pending rows joining the baseline; the bounds stay those of the original baseline."""
    alive = np.ones(len(X), bool) if alive is None else np.array(alive, bool)
    extra = [np.atleast_2d(X_pending)] if X_pending is not None and len(X_pending) else []
    picks, vals = [], []
    for _ in range(q):
        Xb_step = np.vstack([Xb] + extra)
        v = np.full(len(X), -np.inf)
        v[alive] = scores(models, signs, Xb_step, base_samples(S, len(Xb_step), len(models), seed), X[alive], w, lo, hi)[0]
        i = int(np.argmax(v))
        picks.append(i), vals.append(float(v[i]))
        alive[i] = False
        extra.append(X[i][None, :])
    return picks, vals


# ---- plain qNEHVI ------------------------------------------------------------------------------------------------------------------
def qnehvi_scores(models, signs, Xb, ref_point, z, X):
    """mean_s sum_cells prod_o max(min(f_s,o, up_o) - lo_o, 0) with qLogNEHVI's per-sample cells."""
    signs = np.asarray(signs, dtype=np.float64)
    orc = no.NEHVIOracle(models, signs, Xb, ref_point, z)
    out = []
    for x in np.atleast_2d(X):
        f = orc.candidate_samples(x) * signs[None, :]
        out.append(np.mean([no.hvi_from_cells(f[s], *orc.cells[s]) for s in range(len(f))]))
    return np.array(out)


def qnehvi_greedy(models, signs, Xb, ref_point, X, q, S, seed, X_pending=None):
    alive = np.ones(len(X), bool)
    extra = [np.atleast_2d(X_pending)] if X_pending is not None and len(X_pending) else []
    picks, vals = [], []
    for _ in range(q):
        Xb_step = np.vstack([Xb] + extra)
        v = np.full(len(X), -np.inf)
        v[alive] = qnehvi_scores(models, signs, Xb_step, ref_point, base_samples(S, len(Xb_step), len(models), seed), X[alive])
        i = int(np.argmax(v))
        picks.append(i), vals.append(float(v[i]))
        alive[i] = False
        extra.append(X[i][None, :])
    return picks, vals
