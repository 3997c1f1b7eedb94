"""TEST INFRASTRUCTURE - qNEI / qLogNEI restated on the frozen oracle (``oracle/nehvi_oracle.py`` with ONE target).

BoTorch's noisy expected improvement draws f(x) jointly with the baseline values through the cached baseline factor and scores the
improvement over each sample's own best baseline value; ``NEHVIOracle([model], [sign], X_b, ref_point=[-1e9], z)`` already holds both
halves: ``obj_b[:, :, 0].max(1)`` is the per-sample best and ``candidate_samples(x)[:, 0] * sign`` the joint draw."""

import numpy as np

from oracle import gp_oracle as go
from oracle import nehvi_oracle as no

PRUNE_SAMPLES = 2048


def base_samples(S, nb, seed):
    """[S, nb + 1, 1]: one scrambled-Sobol draw of dimension nb + 1, the candidate's column last."""
    return no.sobol_normal_base_samples_nd(S, nb + 1, 1, seed)


def scores(model, sign, Xb, z, X, log=True):
    """(scores [len(X)], best_s [S], joint draws [len(X), S]) of the q = 1 t-batches X."""
    orc = no.NEHVIOracle([model], [sign], Xb, [-1e9], z)
    best = orc.obj_b[:, :, 0].max(1)
    f = np.array([orc.candidate_samples(x)[:, 0] * sign for x in np.atleast_2d(X)])
    u = f - best[None, :]
    if log:
        val = np.array([no.logmeanexp_with_neginf(go.log_fatplus(ui, no.TAU_RELU)) for ui in u])
    else:
        val = np.maximum(u, 0.0).mean(1)
    return val, best, f


def prune(model, sign, Xb, seed):
    """``prune_inferior_points``: indices of the baseline rows that are the best of at least one of 2048 joint draws (ascending),
    and the smallest gap between a sample's best and second-best value."""
    mu, cov = model.posterior_joint(Xb)
    z = go.sobol_normal_base_samples(PRUNE_SAMPLES, len(Xb), seed)
    F = (mu[None, :] + z @ go._safe_cholesky(cov).T) * sign
    top2 = np.sort(F, axis=1)[:, -2:]
    return np.unique(F.argmax(1)), float((top2[:, 1] - top2[:, 0]).min()) if F.shape[1] > 1 else np.inf


def greedy(model, sign, Xb, X, q, S, seed, X_pending=None, log=True, alive=None):
    """Sequential greedy with picks and pending rows joining the baseline (``set_X_pending`` with a cached root)."""
    alive = np.ones(len(X), bool) if alive is None else np.array(alive, bool)
    extra = [np.atleast_2d(X_pending)] if X_pending is not None and len(X_pending) else []
    picks, vals = [], []
    for _ in range(q):
        Xb_step = np.vstack([Xb] + extra)
        v = np.full(len(X), -np.inf)
        v[alive] = scores(model, sign, Xb_step, base_samples(S, len(Xb_step), seed), X[alive], log)[0]
        i = int(np.argmax(v))
        picks.append(i), vals.append(float(v[i]))
        alive[i] = False
        extra.append(X[i][None, :])
    return picks, vals
