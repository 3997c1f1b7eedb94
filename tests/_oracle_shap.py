"""TEST INFRASTRUCTURE - the Shapley oracle (numpy only): every composed row is built explicitly, f is any row function (for a GP the
oracle model's ``posterior(rows)[0]``), v is the mean over the background rows and phi the subset formula

    phi_g = sum over S in G \\ {g} of |S|! (M - |S| - 1)! / M! [v(S + g) - v(S)].

Bit g of a coalition's index stands for feature g; a column in no feature (group -1) keeps the background row's value.
``permutation_shapley`` is the other definition - the marginal contribution averaged over all M! orders - and guards the subset
formula in tests/test_shap_cpu.py."""

from __future__ import annotations

import itertools
import math
from types import SimpleNamespace

import numpy as np

EPS = np.finfo(np.float64).eps


def compose_rows(x: np.ndarray, Bg: np.ndarray, groups: np.ndarray, M: int, masks=None) -> np.ndarray:
    """[len(masks), B, d]: for every coalition the B rows that take x on the coalition's columns and the background row elsewhere."""
    masks = np.arange(1 << M, dtype=np.int64) if masks is None else np.asarray(masks, dtype=np.int64)
    groups = np.asarray(groups)
    take = np.zeros((len(masks), len(groups)), dtype=bool)
    for j, g in enumerate(groups):
        if g >= 0:
            take[:, j] = (masks >> int(g)) & 1
    return np.where(take[:, None, :], x[None, None, :], Bg[None, :, :])


def coalition_values(f, X: np.ndarray, Bg: np.ndarray, groups, M: int, mask_chunk: int = 4096) -> np.ndarray:
    """v [R, 2^M] = mean over b of f(composed rows)."""
    X, Bg = np.atleast_2d(X), np.atleast_2d(Bg)
    B, d = Bg.shape
    v = np.empty((X.shape[0], 1 << M))
    for r in range(X.shape[0]):
        for m0 in range(0, 1 << M, mask_chunk):
            masks = np.arange(m0, min(m0 + mask_chunk, 1 << M))
            rows = compose_rows(X[r], Bg, groups, M, masks).reshape(-1, d)
            v[r, masks] = np.asarray(f(rows)).reshape(len(masks), B).mean(axis=1)
    return v


def subset_shapley(v: np.ndarray, M: int) -> np.ndarray:
    """phi [R, M] from v [R, 2^M] by the subset formula."""
    v = np.atleast_2d(v)
    S = np.arange(1 << M, dtype=np.int64)
    size = np.zeros(1 << M, dtype=np.int64)
    for g in range(M):
        size += (S >> g) & 1
    fact = [math.factorial(k) for k in range(M + 1)]
    phi = np.empty((v.shape[0], M))
    for g in range(M):
        without = S[((S >> g) & 1) == 0]
        w = np.array([fact[k] * fact[M - k - 1] / fact[M] for k in size[without]])
        phi[:, g] = ((v[:, without | (1 << g)] - v[:, without]) * w).sum(axis=1)
    return phi


def permutation_shapley(v: np.ndarray, M: int) -> np.ndarray:
    """phi [R, M]: the marginal contribution of each feature averaged over all M! orders of arrival."""
    v = np.atleast_2d(v)
    phi = np.zeros((v.shape[0], M))
    for order in itertools.permutations(range(M)):
        S = 0
        for g in order:
            phi[:, g] += v[:, S | (1 << g)] - v[:, S]
            S |= 1 << g
    return phi / math.factorial(M)


def explain(om, X, Bg, groups, M: int, kmax: float | None = None):
    """v, phi, base of an oracle GP (``oracle.gp_oracle.GPModel``) with the bound the device is held to at c = 1:
    ``tol_v = (n + M + 16) eps ysd kmax sum_t |alpha_t|`` - a kernel value is at most ``kmax`` (the outputscale, for a composite
    or multi-task kernel the largest prior variance) and the rounding of d2 perturbs it by at most M eps relatively - and
    ``tol_phi = 2 tol_v``."""
    from oracle import gp_oracle as go

    v = coalition_values(lambda rows: om.posterior(rows)[0], X, Bg, groups, M)
    phi = subset_shapley(v, M)
    if kmax is None:
        allrows = np.vstack([np.atleast_2d(X), np.atleast_2d(Bg), om.X_train])
        kmax = float(go.prior_var(om.spec, om.params, go.normalize_inputs(om.spec, allrows)).max())
    n = om.X_train.shape[0]
    tol_v = (n + M + 16) * EPS * om.ysd * kmax * float(np.abs(om.alpha).sum())
    return SimpleNamespace(v=v, phi=phi, base=float(v[0, 0]), tol_v=tol_v, tol_phi=2.0 * tol_v, kmax=kmax)
