"""TEST INFRASTRUCTURE - numpy restatement of qNegIntegratedPosteriorVariance on ``oracle.gp_oracle`` (``GPModel``, ``cross_cov``), in
two independent forms.  [UPSTREAM] BoTorch is restated from memory (``baybe_amd/nipv.py``): the GP is conditioned on the t-batch
``[x ; B]`` with the likelihood's noise at the new points, the latent variance is read at the integration points P, the value is
``-mean_j var_j``.

(a) ``direct``: the GP conditioned on ``X u B u {x}`` by Cholesky of the (n + b + 1)-point noisy covariance, the candidate last.  With
    ``W = L_Z^-1 K(Z, P)`` the variance at p_j is ``k(p_j, p_j) - sum_rows W[:, j]^2``; the rows of W that belong to ``X u B`` do not depend
    on x, so the candidate's contribution is its own row: ``gain(x) = sum_j W[last, j]^2`` - the same factorisation, read without
    subtracting two nearly equal variances.  The factor of ``X u B`` is shared by all candidates (block row of the Cholesky).
(b) ``schur``: the form the kernel evaluates, from posterior covariances given the training data alone:
    ``C_j = cov(x, p_j) - cov(x, B) H[:, j]``, ``gain = sum_j C_j^2 / (max(var(x) - cov(x, B) G^-1 cov(B, x), 0) + s2)``.

``schur`` also returns the first-order bound of the issue, per candidate, at c = 1:
    tol = (n + b + 16) eps [2 sum_j |C_j| S_j + gain D] / den
    S_j = |k(x, p_j)| + sum_r |k*_r A_rj| + sum_l |cov(x, B)_l H_lj|,   D = |var(x)| + sum_lm |cov(x, B)_l G^-1_lm cov(B, x)_m| + s2
Everything is in the target's original scale."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go

EPS = np.finfo(np.float64).eps


def _norm(model, X):
    return go.normalize_inputs(model.spec, np.atleast_2d(np.asarray(X, dtype=np.float64)))


def _k(model, A, B):
    return go.cross_cov(model.spec, model.params, _norm(model, A), _norm(model, B))


def noise(model) -> float:
    return float(model.params.noise)


def condition_number(model) -> float:
    """cond(K + s2 I) of the training covariance (standardised units)."""
    Ky = model.L @ model.L.T
    w = np.linalg.eigvalsh(Ky)
    return float(w[-1] / w[0])


def direct(model, Xc, B, P):
    """Form (a): ``gain`` [N], ``value`` [N] = qNIPV([x ; B]), ``V_B``, ``den`` [N]."""
    Xc, P = np.atleast_2d(Xc), np.atleast_2d(P)
    y2, s2n = model.ysd**2, noise(model)
    Z = model.X_train if B is None or len(B) == 0 else np.vstack([model.X_train, np.atleast_2d(B)])
    Kz = _k(model, Z, Z) + s2n * np.eye(len(Z))
    Lz = sla.cholesky(Kz, lower=True)
    Wz = sla.solve_triangular(Lz, _k(model, Z, P), lower=True)  # [n + b, M]
    var_b = np.diag(_k(model, P, P)) - (Wz * Wz).sum(axis=0)  # var(p_j | X u B), standardised
    lc = sla.solve_triangular(Lz, _k(model, Z, Xc), lower=True)  # [n + b, N]: the candidate's row of the extended factor
    lam2 = np.diag(_k(model, Xc, Xc)) + s2n - (lc * lc).sum(axis=0)
    wlast = (_k(model, Xc, P) - lc.T @ Wz) / np.sqrt(lam2)[:, None]  # [N, M]
    gain = y2 * (wlast * wlast).sum(axis=1)
    v_b = y2 * float(np.mean(var_b))
    value = -y2 * np.mean(var_b[None, :] - wlast * wlast, axis=1)
    return SimpleNamespace(gain=gain, value=value, v_b=v_b, den=y2 * lam2)


def schur(model, Xc, B, P):
    """Form (b) and the bound at c = 1: ``gain``, ``value``, ``V_B``, ``den``, ``tol`` [N]; ``var_p`` [M], ``H`` [b, M], ``ginv`` [b, b]."""
    Xc, P = np.atleast_2d(Xc), np.atleast_2d(P)
    n = len(model.X_train)
    b = 0 if B is None else len(B)
    y2 = model.ysd**2
    s2 = y2 * noise(model)
    L = model.L
    Vc = sla.solve_triangular(L, _k(model, model.X_train, Xc), lower=True)  # [n, N]
    Vp = sla.solve_triangular(L, _k(model, model.X_train, P), lower=True)  # [n, M]
    kxp = y2 * _k(model, Xc, P)
    A = sla.solve_triangular(L.T, Vp, lower=False)  # (K + s2 I)^-1 K(X, P)  [n, M]
    kstar = y2 * _k(model, Xc, model.X_train)  # [N, n]
    var_x = y2 * (np.diag(_k(model, Xc, Xc)) - (Vc * Vc).sum(axis=0))
    var_p = y2 * (np.diag(_k(model, P, P)) - (Vp * Vp).sum(axis=0))
    C = kxp - kstar @ A
    S = np.abs(kxp) + np.abs(kstar) @ np.abs(A)
    q = np.zeros(len(Xc))
    D = np.abs(var_x) + s2
    H = ginv = None
    v_b = float(np.mean(var_p))
    if b:
        Vb = sla.solve_triangular(L, _k(model, model.X_train, B), lower=True)  # [n, b]
        cov_xb = y2 * (_k(model, Xc, B) - Vc.T @ Vb)  # [N, b]
        cov_bp = y2 * (_k(model, B, P) - Vb.T @ Vp)  # [b, M]
        G = y2 * (_k(model, B, B) - Vb.T @ Vb) + s2 * np.eye(b)
        ginv = np.linalg.inv(G)
        ginv = 0.5 * (ginv + ginv.T)
        H = ginv @ cov_bp
        C = C - cov_xb @ H
        S = S + np.abs(cov_xb) @ np.abs(H)
        q = np.einsum("il,lm,im->i", cov_xb, ginv, cov_xb)
        D = D + np.einsum("il,lm,im->i", np.abs(cov_xb), np.abs(ginv), np.abs(cov_xb))
        v_b = float(np.mean(var_p - np.einsum("lj,lj->j", cov_bp, H)))
    den = np.maximum(var_x - q, 0.0) + s2
    gain = (C * C).sum(axis=1) / den
    tol = (n + b + 16) * EPS * (2.0 * (np.abs(C) * S).sum(axis=1) + gain * D) / den
    return SimpleNamespace(gain=gain, value=gain / P.shape[0] - v_b, v_b=v_b, den=den, tol=tol, var_p=var_p, var_x=var_x, H=H, ginv=ginv)


def greedy(model, Xc, q, P, pending=None, alive=None):
    """Greedy picks on form (a)'s gain, first index on ties: per step (index, gain of the pick, top-two gap, tol(c = 1) of the top two
    rows summed, the pending rows the step conditioned on)."""
    Xc = np.atleast_2d(Xc)
    alive = np.ones(len(Xc), dtype=bool) if alive is None else np.array(alive, dtype=bool)
    base = np.zeros((0, Xc.shape[1])) if pending is None or len(pending) == 0 else np.atleast_2d(pending)
    rows, steps = [], []
    for _ in range(q):
        pend = np.vstack([base] + rows) if rows else base
        g = np.where(alive, direct(model, Xc, pend, P).gain, -np.inf)
        tol = schur(model, Xc, pend, P).tol
        order = np.argsort(-g, kind="stable")
        i0, i1 = int(order[0]), int(order[1])
        steps.append(SimpleNamespace(index=i0, gain=float(g[i0]), gap=float(g[i0] - g[i1]), tol2=float(tol[i0] + tol[i1]), pending=pend))
        alive[i0] = False
        rows.append(Xc[i0 : i0 + 1])
    return steps
