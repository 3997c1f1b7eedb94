"""Gradient-based refinement of continuous coordinates: a batched maximiser over a box (``maximize_box``) or over a polytope known
through its projection (``maximize_polytope``).

The reference refines its raw samples with L-BFGS-B, one SciPy run per restart, through autograd gradients
(``optimize_acqf`` / ``optimize_acqf_mixed``; botorch/hybrid.py:95-136).  On the device path the acquisition value AND its
gradient of every start come out of one pass (``HipGP.qlogei_value_grad``), so the optimiser below advances all starts together:
one callback call per trial, however many starts there are.  It is a pure numpy function of its callback.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ARMIJO_C1 = 1e-4
MAX_BACKTRACKS = 20


@dataclass
class BoxResult:
    x: np.ndarray  # [k, d] final points
    values: np.ndarray  # [k] their values (a frozen start: the best value it reached)
    iterations: int  # outer iterations; the evaluation of the starts is the first
    backtracks: int  # further callback calls spent on Armijo backtracking
    calls: int  # callback calls in all = iterations + backtracks
    converged: np.ndarray  # [k] bool: projected gradient below gtol, or no further progress possible
    ok: np.ndarray  # [k] bool: False for a start the callback flagged at its start point


def _two_loop(g, S, Y, rho, free):
    """H g of every start from its own L-BFGS history (pairs with rho = 0 are empty slots), on the free coordinates."""
    q = np.where(free, g, 0.0)
    m = S.shape[1]
    a = np.zeros((m, g.shape[0]))
    for j in range(m - 1, -1, -1):
        a[j] = rho[:, j] * np.einsum("kd,kd->k", S[:, j], q)
        q = q - a[j][:, None] * Y[:, j]
    yy = np.einsum("kd,kd->k", Y[:, -1], Y[:, -1])
    sy = np.einsum("kd,kd->k", S[:, -1], Y[:, -1])
    gamma = np.where((rho[:, -1] > 0) & (yy > 0), sy / np.where(yy > 0, yy, 1.0), 1.0)
    r = gamma[:, None] * q
    for j in range(m):
        b = rho[:, j] * np.einsum("kd,kd->k", Y[:, j], r)
        r = r + S[:, j] * (a[j] - b)[:, None]
    return np.where(free, r, 0.0)


def maximize_box(value_and_grad, starts, lo, hi, *, max_iter: int = 200, gtol: float = 1e-10, memory: int = 8) -> BoxResult:
    """Maximise ``f`` over the box [lo, hi] from every row of ``starts`` [k, d] at once.

    ``value_and_grad(X [k, d]) -> (values [k], grads [k, d], ok [k])`` is called ONCE per trial with all starts (a frozen start
    is passed at its resting point).  Every start keeps its own step length and its own L-BFGS history (``memory`` pairs) and
    takes projected steps x <- clip(x + t d) with Armijo backtracking on t.  A start is frozen at its best point once its
    projected gradient is below ``gtol`` (max norm), once a step's predicted gain is below the rounding of the value or
    backtracking finds no improvement, or when the callback returns
    ``ok = 0`` for it (such a trial is never accepted; flagged at its start, it keeps its start value)."""
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    x = np.clip(np.array(starts, dtype=np.float64, copy=True).reshape(-1, lo.shape[0]), lo, hi)
    k, d = x.shape
    span = np.where(hi > lo, hi - lo, 1.0)
    calls = 0

    def evaluate(X):
        nonlocal calls
        calls += 1
        f, g, ok = value_and_grad(X)
        f = np.asarray(f, dtype=np.float64).reshape(k)
        g = np.asarray(g, dtype=np.float64).reshape(k, d)
        ok = np.asarray(ok).reshape(k).astype(bool) & np.isfinite(f) & np.isfinite(g).all(axis=1)
        return f, g, ok

    f, g, ok0 = evaluate(x)
    iterations, backtracks = 1, 0
    active = ok0.copy()
    converged = np.zeros(k, dtype=bool)
    S = np.zeros((k, memory, d))
    Y = np.zeros((k, memory, d))
    rho = np.zeros((k, memory))
    step = np.full(k, 0.1)  # steepest-ascent step of a start without history, as a fraction of the box
    while iterations < max_iter:
        free = ~(((x <= lo) & (g < 0)) | ((x >= hi) & (g > 0)))
        pg = np.where(free, g, 0.0)
        done = active & (np.abs(pg).max(axis=1) <= gtol)
        converged |= done
        active &= ~done
        if not active.any():
            break
        dirn = _two_loop(g, S, Y, rho, free)
        has_hist = rho.max(axis=1) > 0
        slope = np.einsum("kd,kd->k", dirn, pg)
        use_sd = ~has_hist | ~(slope > 0) | ~np.isfinite(dirn).all(axis=1)
        rho[use_sd & has_hist] = 0.0  # a history that gives no ascent direction is dropped
        scale = np.abs(pg / span).max(axis=1)
        sd = pg * (step / np.where(scale > 0, scale, 1.0))[:, None]
        dirn = np.where(use_sd[:, None], sd, dirn)
        # no measurable progress left: the first trial's predicted gain is below the rounding of the value itself
        predicted = np.einsum("kd,kd->k", g, np.clip(x + dirn, lo, hi) - x)
        flat = active & ~(predicted > 8.0 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(f)))
        converged |= flat
        active &= ~flat
        if not active.any():
            break
        t = np.ones(k)
        pending = active.copy()  # starts still looking for an acceptable trial in this iteration
        x_new, f_new, g_new = x.copy(), f.copy(), g.copy()
        accepted = np.zeros(k, dtype=bool)
        first = True
        for _ in range(MAX_BACKTRACKS + 1):
            trial = np.where(pending[:, None], np.clip(x + t[:, None] * dirn, lo, hi), x)
            ft, gt, okt = evaluate(trial)
            if first:
                iterations += 1
                first = False
            else:
                backtracks += 1
            flagged = pending & ~okt  # the callback cannot differentiate there: the start rests at its best point
            active &= ~flagged
            pending &= ~flagged
            gain = np.einsum("kd,kd->k", g, trial - x)
            good = pending & (ft >= f + ARMIJO_C1 * gain) & (ft > f)
            x_new[good], f_new[good], g_new[good] = trial[good], ft[good], gt[good]
            accepted |= good
            pending &= ~good
            if not pending.any():
                break
            t[pending] *= 0.5
        stalled = pending  # no acceptable trial: with a history, try again from steepest ascent; without, the start is done
        drop = stalled & has_hist & ~use_sd
        rho[drop] = 0.0
        finished = stalled & ~drop
        converged |= finished
        active &= ~finished
        # per-start step length of the steepest-ascent fallback: what was accepted, doubled
        step = np.where(accepted & use_sd, np.minimum(2.0 * step * t, 1.0), step)
        step = np.where(finished, step, np.maximum(step, 1e-12))
        s = x_new - x
        y = g - g_new  # gradient change of -f
        sy = np.einsum("kd,kd->k", s, y)
        keep = accepted & (sy > 1e-12 * np.sqrt(np.einsum("kd,kd->k", s, s) * np.einsum("kd,kd->k", y, y)))
        if keep.any():
            S[keep, :-1], Y[keep, :-1], rho[keep, :-1] = S[keep, 1:], Y[keep, 1:], rho[keep, 1:]
            S[keep, -1], Y[keep, -1], rho[keep, -1] = s[keep], y[keep], 1.0 / sy[keep]
        x, f, g = x_new, f_new, g_new
    return BoxResult(x=x, values=f, iterations=iterations, backtracks=backtracks, calls=calls, converged=converged, ok=ok0)


def maximize_polytope(value_and_grad, starts, project, *, max_iter: int = 200, gtol: float = 1e-10, memory: int = 8) -> BoxResult:
    """``maximize_box`` over a polytope that is known through its Euclidean projection only: the same scheme - per-start L-BFGS
    history, Armijo backtracking, ONE ``value_and_grad`` call per trial with all starts - with ``project`` where ``maximize_box``
    clips.

    ``project(X [k, d]) -> (X' [k, d], ok [k])`` is called with all starts at once (a frozen start is passed too; its row is
    ignored).  The trial of a start is ``project(x + t d)``, its Armijo gain ``g . (trial - x)``.  If the L-BFGS direction gives
    ``g . (project(x + d) - x) <= 0`` the start drops its history and falls back to the steepest arc ``project(x + t g)``, whose
    first ``t`` moves it by a tenth of its projected-gradient step and doubles with every accepted trial.  A start has converged once
    ``|project(x + g) - x|_inf <= gtol``, or once the predicted gain of its first trial is below the rounding of the value (it
    takes that trial if the value does not measurably fall).  The L-BFGS pairs are (step, change of the PROJECTED gradient
    ``project(x + g) - x``): both lie in the face the start moves on, whereas the raw gradient keeps the components normal to it,
    which every projection removes again.  A start whose projection reports ``ok = 0`` - at its start (it then rests there), in a
    trial or in one of the tests above - is frozen at its best point, as one the callback flags."""
    x0 = np.array(starts, dtype=np.float64, copy=True)
    x0 = x0.reshape(-1, x0.shape[-1]) if x0.ndim > 1 else x0.reshape(1, -1)
    k, d = x0.shape
    calls = 0

    def proj(X):
        P, okp = project(X)
        return np.asarray(P, dtype=np.float64).reshape(k, d), np.asarray(okp).reshape(k).astype(bool)

    def evaluate(X):
        nonlocal calls
        calls += 1
        f, g, ok = value_and_grad(X)
        f = np.asarray(f, dtype=np.float64).reshape(k)
        g = np.asarray(g, dtype=np.float64).reshape(k, d)
        ok = np.asarray(ok).reshape(k).astype(bool) & np.isfinite(f) & np.isfinite(g).all(axis=1)
        return f, g, ok

    xp, okp0 = proj(x0)
    x = np.where(okp0[:, None], xp, x0)
    f, g, ok0 = evaluate(x)
    ok0 &= okp0
    iterations, backtracks = 1, 0
    active = ok0.copy()
    converged = np.zeros(k, dtype=bool)
    S = np.zeros((k, memory, d))
    Y = np.zeros((k, memory, d))
    rho = np.zeros((k, memory))
    step = np.zeros(k)  # multiple of g of the steepest arc's first trial; 0: not chosen yet
    everywhere = np.ones((k, d), dtype=bool)
    prev = None  # (point, projected gradient, accepted) of the iteration before
    dot = lambda a, b: np.einsum("kd,kd->k", a, b)  # noqa: E731
    while iterations < max_iter:
        gsafe = np.where(active[:, None], g, 0.0)
        xg, okg = proj(x + gsafe)
        pg = np.where(active[:, None], xg - x, 0.0)
        active &= okg
        pgn = np.abs(pg).max(axis=1)
        done = active & (pgn <= gtol)
        converged |= done
        active &= ~done
        if not active.any():
            break
        if prev is not None:
            # the history lives in the face the start moves on: s between two accepted points, y the change of the PROJECTED
            # gradient (that of g itself carries the components normal to the face, which the projection removes from every step)
            x_old, pg_old, took = prev
            s = x - x_old
            y = pg_old - pg  # projected-gradient change of -f
            sy = dot(s, y)
            keep = took & active & (sy > 1e-12 * np.sqrt(dot(s, s) * dot(y, y)))
            if keep.any():
                S[keep, :-1], Y[keep, :-1], rho[keep, :-1] = S[keep, 1:], Y[keep, 1:], rho[keep, 1:]
                S[keep, -1], Y[keep, -1], rho[keep, -1] = s[keep], y[keep], 1.0 / sy[keep]
        dirn = _two_loop(pg, S, Y, rho, everywhere)
        has_hist = rho.max(axis=1) > 0
        fin = np.isfinite(dirn).all(axis=1)
        xd, okd = proj(x + np.where((active & has_hist & fin)[:, None], dirn, 0.0))
        slope = dot(g, xd - x)
        use_sd = ~has_hist | ~(slope > 0) | ~fin | ~okd
        rho[use_sd & has_hist] = 0.0  # a history that gives no ascent direction is dropped
        gn = np.abs(g).max(axis=1)
        fresh = step <= 0
        step = np.where(fresh, 0.1 * pgn / np.where(gn > 0, gn, 1.0), step)
        dirn = np.where(use_sd[:, None], g * step[:, None], dirn)
        dirn = np.where(active[:, None], dirn, 0.0)
        t = np.ones(k)
        pending = active.copy()  # starts still looking for an acceptable trial in this iteration
        x_new, f_new, g_new = x.copy(), f.copy(), g.copy()
        accepted = np.zeros(k, dtype=bool)
        first = True
        for _ in range(MAX_BACKTRACKS + 1):
            xt, okt_p = proj(x + t[:, None] * dirn)
            trial = np.where(pending[:, None], xt, x)
            gain = dot(g, trial - x)
            if first:
                # no measurable progress left: the first trial's predicted gain is below the rounding of the value itself.  Such a
                # start is done, but its trial rides along in this evaluation and is taken if the value does not measurably fall:
                # the value no longer tells the points apart, while the step still shortens the projected gradient
                noise = 8.0 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(f))
                flat = pending & okt_p & ~(gain > noise)
                pending &= ~flat
                trial = np.where((pending | flat)[:, None], xt, x)
            ft, gt, okt = evaluate(trial)
            if first:
                iterations += 1
                first = False
                last = flat & okt & (ft >= f - noise)
                x_new[last], f_new[last], g_new[last] = trial[last], ft[last], gt[last]
                converged |= flat
                active &= ~flat
            else:
                backtracks += 1
            flagged = pending & ~(okt & okt_p)  # no projection, or no derivative there: the start rests at its best point
            active &= ~flagged
            pending &= ~flagged
            good = pending & (ft >= f + ARMIJO_C1 * gain) & (ft > f)
            x_new[good], f_new[good], g_new[good] = trial[good], ft[good], gt[good]
            accepted |= good
            pending &= ~good
            if not pending.any():
                break
            t[pending] *= 0.5
        stalled = pending  # no acceptable trial: with a history, try again from the steepest arc; without, the start is done
        drop = stalled & has_hist & ~use_sd
        rho[drop] = 0.0
        finished = stalled & ~drop
        converged |= finished
        active &= ~finished
        # per-start length of the steepest arc: what was accepted, doubled
        step = np.where(accepted & use_sd, 2.0 * step * t, step)
        prev = (x, pg, accepted)
        x, f, g = x_new, f_new, g_new
    return BoxResult(x=x, values=f, iterations=iterations, backtracks=backtracks, calls=calls, converged=converged, ok=ok0)
