"""Closed-form oracle of the posterior derivatives with respect to a candidate (numpy), and the finite-difference criterion the
derivative tests share.

    k*_i = os kappa(r_i),   g_ij = d k*_i / d x_j  (raw coordinate; r-free form):
      matern32  -3 os exp(-sqrt3 r) D_ij / l_j^2       matern52  -(5/3) os (1 + sqrt5 r) exp(-sqrt5 r) D_ij / l_j^2
      rbf       -k*_i D_ij / l_j^2                     D_ij = xn_j - Xn_ij (normalised), d xn_j / d x_j = 1 / (hi_j - lo_j)
    w = (K + s2 I)^-1 k*;  d mean_j = ysd sum_i alpha_i g_ij;  d var_j = -2 ysd^2 sum_i w_i g_ij;
    d cross_rj = ysd^2 (d k(x, p_r) / d x_j - sum_i beta_ri g_ij),  beta_r = (K + s2 I)^-1 k(X, p_r).

Every derivative comes with ``S_abs``, the sum of the absolute values of its terms as formed here: the scale a bound of the form
c (n + 16) eps S_abs refers to.
"""

from __future__ import annotations

import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go

EPS = np.finfo(np.float64).eps


def _kernel_and_factor(kernel: str, r2: np.ndarray, os: float):
    r = np.sqrt(np.maximum(r2, 1e-30))
    if kernel == "rbf":
        k = os * np.exp(-0.5 * r2)
        return k, -k
    if kernel == "matern52":
        e = np.exp(-math.sqrt(5.0) * r)
        return os * (1.0 + math.sqrt(5.0) * r + (5.0 / 3.0) * r * r) * e, -(5.0 / 3.0) * os * (1.0 + math.sqrt(5.0) * r) * e
    if kernel == "matern32":
        e = np.exp(-math.sqrt(3.0) * r)
        return os * (1.0 + math.sqrt(3.0) * r) * e, -3.0 * os * e
    raise ValueError(kernel)


def _g(model, Xcn: np.ndarray, Bn: np.ndarray, cols_num: np.ndarray):
    """k(x_c, b_i) [N, m] and g [N, m, dc] = d k(x_c, b_i) / d (raw x_c,j) for the numerical positions ``cols_num``."""
    spec, prm = model.spec, model.params
    ls = np.asarray(prm.lengthscale, dtype=float)
    os = prm.outputscale if spec.use_outputscale else 1.0
    A, B = Xcn[:, spec.num_idx], Bn[:, spec.num_idx]
    r2 = go._scaled_sqdist(A, B, ls)
    k, gf = _kernel_and_factor(spec.kernel, r2, os)
    D = A[:, None, cols_num] - B[None, :, cols_num]  # [N, m, dc]
    rng = (spec.hi - spec.lo)[cols_num]
    return k, gf[:, :, None] * D / (ls[cols_num] ** 2) / rng


def posterior_grad_oracle(model, X: np.ndarray, cols, pend: np.ndarray | None = None) -> dict:
    """mean / var / cross and their derivatives at the rows of X (raw comp-rep) with respect to the comp-rep columns ``cols``;
    ``pend`` [p, d] raw pending rows (None: no cross outputs).  Keys: mean, var, cross, dmean, dvar, dcross and, for the three
    derivatives, S_dmean, S_dvar, S_dcross."""
    spec = model.spec
    X = np.atleast_2d(np.asarray(X, dtype=float))
    num = list(np.asarray(spec.num_idx))
    cols_num = np.array([num.index(int(c)) for c in cols], dtype=np.int64)
    Xcn = go.normalize_inputs(spec, X)
    k, g = _g(model, Xcn, model.Xn, cols_num)  # [N, n], [N, n, dc]
    W = sla.cho_solve((model.L, True), k.T).T  # [N, n]
    s1, s2 = model.ysd, model.ysd**2
    os = model.params.outputscale if spec.use_outputscale else 1.0
    out = {
        "mean": model.ybar + s1 * (model.params.mean + k @ model.alpha),
        "var": s2 * (os - np.einsum("ni,ni->n", k, W)),
        "dmean": s1 * np.einsum("i,nij->nj", model.alpha, g),
        "S_dmean": s1 * np.einsum("i,nij->nj", np.abs(model.alpha), np.abs(g)),
        "dvar": -2.0 * s2 * np.einsum("ni,nij->nj", W, g),
        "S_dvar": 2.0 * s2 * np.einsum("ni,nij->nj", np.abs(W), np.abs(g)),
    }
    if pend is not None and len(pend):
        Pn = go.normalize_inputs(spec, np.atleast_2d(np.asarray(pend, dtype=float)))
        kp, gp = _g(model, Xcn, Pn, cols_num)  # [N, p], [N, p, dc]
        KP = go.cross_cov(spec, model.params, Pn, model.Xn)  # [p, n]
        beta = sla.cho_solve((model.L, True), KP.T).T  # [p, n]
        out["cross"] = s2 * (kp - k @ beta.T)
        out["dcross"] = s2 * (gp - np.einsum("ri,nij->nrj", beta, g))
        out["S_dcross"] = s2 * (np.abs(gp) + np.einsum("ri,nij->nrj", np.abs(beta), np.abs(g)))
    return out


def two_step_ok(g, fd_h, fd_h2, f, h):
    """|g - FD_{h/2}| <= |FD_h - FD_{h/2}| + 16 eps |f| / h, elementwise: (holds, |g - FD_{h/2}|, bound)."""
    err = np.abs(np.asarray(g) - fd_h2)
    bound = np.abs(fd_h - fd_h2) + 16.0 * EPS * np.abs(f) / h
    return err <= bound, err, bound


def central_difference(fun, x: np.ndarray, j: int, h: float):
    """(fun(x + h e_j) - fun(x - h e_j)) / (2 h) for a function of one row."""
    xp, xm = np.array(x, dtype=float, copy=True), np.array(x, dtype=float, copy=True)
    xp[j] += h
    xm[j] -= h
    return (np.asarray(fun(xp)) - np.asarray(fun(xm))) / (2.0 * h)
