"""TEST INFRASTRUCTURE - the MC acquisition functions of a transformed target restated in numpy, for tests/test_objective_cpu.py and
tests/test_objective_gpu.py.

A program here is a tuple of (operation name, parameters), interpreted by ``apply_program`` below - written from the operation
definitions of include/baybe_hip.h and deliberately NOT shared with ``baybe_amd/objective.py`` (whose ``ObjectiveProgram.ops`` has
the same layout, so a product program can be handed over as ``prog.ops``).  Scores: per row ``oracle.gp_oracle._safe_cholesky`` of
the joint covariance, ``Y = m + z L^T``, ``G = program(Y)``, then the reduction of the kind - qLogEI as in
``_joint_cases.dense_score`` (log-fat-softplus, fat maximum, log-mean-exp), the others as ``oracle.gp_oracle.mc_acq_joint``.

``ObjectiveOracleEngine`` is ``_oracle_engine.OracleEngine`` with ``mc_acq(..., objective=, stats=)``: the CPU double of the
device for runs of the plug-in with transformed targets."""

from __future__ import annotations

import math

import numpy as np
import torch

from _oracle_engine import OracleEngine
from oracle import gp_oracle as go

MC_KINDS = ("qLogEI", "qEI", "qPI", "qSR", "qUCB", "qPSTD")
TAU_RELU, TAU_MAX = 1e-6, 1e-2


def apply_program(ops, y):
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        for name, p in ops:
            if name == "AFFINE":
                y = p[0] * y + p[1]
            elif name == "CLAMP":
                y = np.clip(y, p[0], p[1])
            elif name == "TWOSIDED":
                y = np.where(y < p[2], p[0] * (y - p[2]), p[1] * (y - p[2]))
            elif name == "BELL":
                y = np.exp(-0.5 * np.square((y - p[0]) / p[1]))
            elif name == "LOG":
                y = np.log(y)
            elif name == "EXP":
                y = np.exp(y)
            elif name == "POW":
                y = y ** int(p[0])
            elif name == "SIGMOID":
                y = 1.0 / (1.0 + np.exp(p[1] * (y - p[0])))
            else:
                raise ValueError(name)
    return y


def _log_fatplus(x):
    t = x / TAU_RELU
    return math.log(TAU_RELU) + np.log(np.logaddexp(0.0, t) + 0.1 / (1.0 + t * t))


def reduce_samples(kind: str, G: np.ndarray, best_f: float, beta: float) -> np.ndarray:
    """G [..., S, q] objective samples -> score [...]."""
    from scipy.special import logsumexp

    if kind == "qLogEI":
        li = _log_fatplus(G - best_f)
        M = li.max(axis=-1, keepdims=True)
        fm = M[..., 0] + TAU_MAX * np.log(((2.0 / (2.0 + (M - li) / TAU_MAX)) ** 2).sum(axis=-1))
        return logsumexp(fm, axis=-1) - math.log(G.shape[-2])
    if kind == "qEI":
        u = np.maximum(G - best_f, 0.0)
    elif kind == "qPI":
        u = 1.0 / (1.0 + np.exp(-(G - best_f) / 1e-3))
    elif kind == "qSR":
        u = G
    else:
        m = G.mean(axis=-2, keepdims=True)
        dev = np.abs(G - m)
        u = m + math.sqrt(beta * math.pi / 2.0) * dev if kind == "qUCB" else math.sqrt(math.pi / 2.0) * dev
    return u.max(axis=-1).mean(axis=-1)


def scores_from_factors(kind, ops, means, L, z, best_f, beta=0.2):
    """means [N, q], L [N, q, q] lower factors, z [S, q] -> [N] (NaN where the factor is NaN)."""
    with np.errstate(all="ignore"):
        Y = means[:, None, :] + np.einsum("sc,nrc->nsr", z, L)
        return reduce_samples(kind, apply_program(ops, Y), best_f, beta)


def q1_scores(kind, ops, mu, var, z, best_f, beta=0.2):
    """N single candidates: 1 x 1 factors with psd_safe_cholesky's jitter (``_safe_sqrt_var``)."""
    sd = go._safe_sqrt_var(np.asarray(var, dtype=np.float64))
    return scores_from_factors(kind, ops, np.asarray(mu, dtype=np.float64)[:, None], sd[:, None, None],
                               np.asarray(z, dtype=np.float64).reshape(-1, 1), best_f, beta)


def lapack_factors(Sig: np.ndarray) -> np.ndarray:
    """``_safe_cholesky`` of every matrix of the stack [N, q, q]; NaN where it raises."""
    import scipy.linalg as sla

    out = np.full_like(Sig, np.nan)
    for i, A in enumerate(Sig):
        try:
            out[i] = go._safe_cholesky(A)
        except sla.LinAlgError:
            pass
    return out


def rowwise_factors(Sig: np.ndarray) -> np.ndarray:
    """The kernels' factorisation (row by row, ascending k, the jitter level ``_joint_cases.unblocked_attempts`` finds) of the stack
    [N, q, q]; NaN where no level succeeds."""
    from _joint_cases import JITTERS, unblocked_attempts

    attempts, done, _ = unblocked_attempts(Sig)
    jit = np.array(JITTERS)[attempts - 1]
    N, q, _ = Sig.shape
    L = np.zeros_like(Sig)
    with np.errstate(all="ignore"):
        for r in range(q):
            for c in range(r + 1):
                s = Sig[:, r, c] + (jit if r == c else 0.0)
                for k in range(c):
                    s = s - L[:, r, k] * L[:, c, k]
                L[:, r, c] = np.sqrt(s) if r == c else s / L[:, c, c]
    L[~done] = np.nan
    return L


def case_sigma(d) -> np.ndarray:
    """[N, q', q'] joint covariances of a ``_joint_cases.JointData`` and [N, q'] joint means."""
    N, p = d.cross.shape
    Sig = np.empty((N, p + 1, p + 1))
    Sig[:, 0, 0] = d.var
    Sig[:, 0, 1:] = Sig[:, 1:, 0] = d.cross
    Sig[:, 1:, 1:] = d.cov_pp
    means = np.concatenate([d.mean[:, None], np.broadcast_to(d.mean_p, (N, p))], axis=1)
    return Sig, means


def joint_scores(kind, ops, mu, var, cross, mp, cpp, z, best_f, beta=0.2, alive=None):
    """[N] scores of the t-batches [x_i ; pending]: -inf for masked rows, NaN where the covariance does not factor."""
    N, p = len(mu), len(mp)
    Sig = np.empty((N, p + 1, p + 1))
    Sig[:, 0, 0], Sig[:, 0, 1:], Sig[:, 1:, 0], Sig[:, 1:, 1:] = var, cross, cross, cpp
    means = np.concatenate([np.asarray(mu)[:, None], np.broadcast_to(mp, (N, p))], axis=1)
    out = scores_from_factors(kind, ops, means, lapack_factors(Sig), z, best_f, beta)
    if alive is not None:
        out = np.where(np.asarray(alive).astype(bool), out, -np.inf)
    return out


class ObjectiveOracleEngine(OracleEngine):
    """``OracleEngine`` that accepts the objective program of ``HipGP.mc_acq`` / ``HipGP.best_f``."""

    def mc_acq(self, kind, mean, var, z, best_f=0.0, sign=1.0, beta=0.2, alive=None, cross=None, objective=None, stats=None):
        if objective is None:
            return super().mc_acq(kind, mean, var, z, best_f, sign, beta, alive, cross)
        mu, v = mean.numpy(), var.numpy()
        z = np.ascontiguousarray(z, dtype=np.float64)
        if cross is None:
            self.calls.append(("mc_acq_obj_q1", kind))
            return self._mask(q1_scores(kind, objective.ops, mu, v, z, best_f, beta), alive)
        mp, cpp = stats if stats is not None else self._pend_stats
        self.calls.append(("mc_acq_obj_pending", kind))
        out = joint_scores(kind, objective.ops, mu, v, cross.numpy(), np.asarray(mp), np.asarray(cpp), z, best_f, beta,
                           None if alive is None else alive.numpy())
        return torch.from_numpy(np.ascontiguousarray(out))


def install(monkeypatch):
    """``_oracle_engine.install`` with ``ObjectiveOracleEngine`` as the engine."""
    import _oracle_engine
    from baybe_amd import engine as engine_mod

    _oracle_engine.install(monkeypatch)
    monkeypatch.setattr(engine_mod, "HipGP", ObjectiveOracleEngine)
    return ObjectiveOracleEngine


# ---- on a fitted oracle model (end-to-end comparisons) ------------------------------------------------------------------------
def model_scores(model, X, pend, ops, kind, z, best_f, beta=0.2):
    """Scores of the t-batches [x_i ; pend] under the oracle model's joint posterior."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    if pend is None or len(pend) == 0:
        mu, var = model.posterior(X)
        return q1_scores(kind, ops, mu, var, np.asarray(z).reshape(-1), best_f, beta)
    N = len(X)
    mu, cov = model.posterior_joint(np.vstack([X, pend]))
    return joint_scores(kind, ops, mu[:N], np.diag(cov)[:N].copy(), cov[:N, N:], mu[N:], cov[N:, N:], z, best_f, beta)


def best_f(model, ops) -> float:
    """max_i program(posterior mean at the training inputs)."""
    return float(apply_program(ops, model.posterior(model.X_train)[0]).max())


def greedy(model, X, q, seed, ops, kind="qLogEI", S=512, beta=0.2, pending=None):
    """Sequential greedy of ``optimize_acqf_discrete`` (first index on ties, picks leave the candidate set): (indices, values)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    bf = best_f(model, ops)
    base = np.zeros((0, X.shape[1])) if pending is None else np.atleast_2d(pending)
    live = np.ones(len(X), dtype=bool)
    idx, vals = [], []
    for _ in range(q):
        pend = np.vstack([base, X[idx]]) if idx else base
        z = go.sobol_normal_base_samples(S, 1 + len(pend), seed)
        s = np.where(live, model_scores(model, X, pend, ops, kind, z, bf, beta), -np.inf)
        i = int(np.argmax(s))
        idx.append(i), vals.append(float(s[i]))
        live[i] = False
    return idx, vals
