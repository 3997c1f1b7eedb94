"""TEST INFRASTRUCTURE - the MC acquisition functions of a desirability objective with one model per target, restated in numpy
for tests/test_desirability_cpu.py and tests/test_desirability_gpu.py.

Deliberately NOT shared with ``baybe_amd/desirability.py``: a description here is a ``Des`` - per target a program as a list of
operation tuples (``_oracle_objective.apply_program``), the normalised weights, the scalariser's name - and the scalarisation is
written out below from the reference's definition (``objectives/desirability.py:41-70, 229-264``).  Scores: per target and row
``_safe_cholesky`` of the joint covariance, ``Y_t = m_t + z[:, :, t] L_t^T``, ``D = scalarise(program_t(Y_t))``, then
``_oracle_objective.reduce_samples`` for the kind.  NaN where ANY target's covariance does not factor.

``DesirabilityOracleEngine`` is ``ObjectiveOracleEngine`` with ``desirability_acq``: the CPU double of the device for runs of the
plug-in under ``desirability="device"``."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

import _oracle_objective as oo
from oracle import gp_oracle as go

EPS = float(np.finfo(np.float64).eps)


class Des(NamedTuple):
    programs: tuple  # per target: tuple of (operation name, parameters)
    weights: tuple   # normalised
    scalarizer: str  # "MEAN" | "GEOM_MEAN"


def from_product(program) -> Des:
    """The data of a product ``DesirabilityProgram`` (read as attributes; nothing of the product is called)."""
    return Des(tuple(tuple(p.ops) for p in program.programs), tuple(program.normalized_weights), str(program.scalarizer))


def desirability(des: Des, Y: np.ndarray) -> np.ndarray:
    """Y [..., T] -> [...]."""
    Y = np.asarray(Y, dtype=np.float64)
    w = np.asarray(des.weights, dtype=np.float64)
    with np.errstate(all="ignore"):
        G = np.stack([oo.apply_program(ops, Y[..., t]) for t, ops in enumerate(des.programs)], axis=-1)
        if des.scalarizer == "GEOM_MEAN":
            return np.exp((np.log(G + EPS) * w).sum(axis=-1))
        if des.scalarizer == "MEAN":
            return (G * w).sum(axis=-1)
    raise ValueError(des.scalarizer)


def scores_from_factors(kind, des: Des, means, L, z, best_f, beta=0.2):
    """means [T, N, q], L [T, N, q, q] lower factors, z [S, q, T] -> [N] (NaN where a factor is NaN)."""
    with np.errstate(all="ignore"):
        Y = np.stack([means[t][:, None, :] + np.einsum("sc,nrc->nsr", z[:, :, t], L[t]) for t in range(len(des.programs))], axis=-1)
        return oo.reduce_samples(kind, desirability(des, Y), best_f, beta)  # [N, S, q, T] -> [N, S, q] -> [N]


def q1_scores(kind, des: Des, mu, var, z, best_f, beta=0.2):
    """mu / var [T, N], z [S, T]: 1 x 1 factors with psd_safe_cholesky's jitter."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    sd = np.stack([go._safe_sqrt_var(v) for v in var])
    return scores_from_factors(kind, des, mu[:, :, None], sd[:, :, None, None], np.asarray(z, dtype=np.float64)[:, None, :], best_f, beta)


def sigma(var, cross, cpp):
    """[N, q, q] joint covariances of one target."""
    N, p = cross.shape
    Sig = np.empty((N, p + 1, p + 1))
    Sig[:, 0, 0], Sig[:, 0, 1:], Sig[:, 1:, 0], Sig[:, 1:, 1:] = var, cross, cross, cpp
    return Sig


def joint_means(mu, mp):
    return np.stack([np.concatenate([m[:, None], np.broadcast_to(q, (len(m), len(q)))], axis=1) for m, q in zip(mu, mp)])


def joint_scores(kind, des: Des, mu, var, cross, mp, cpp, z, best_f, beta=0.2, alive=None):
    """mu / var [T, N], cross [T, N, p], mp [T, p], cpp [T, p, p], z [S, p + 1, T] -> [N]: -inf for masked rows, NaN where a
    target's covariance does not factor."""
    L = np.stack([oo.lapack_factors(sigma(var[t], cross[t], cpp[t])) for t in range(len(des.programs))])
    out = scores_from_factors(kind, des, joint_means(mu, mp), L, z, best_f, beta)
    if alive is not None:
        out = np.where(np.asarray(alive).astype(bool), out, -np.inf)
    return out


class DesirabilityOracleEngine(oo.ObjectiveOracleEngine):
    """``ObjectiveOracleEngine`` that accepts ``HipGP.desirability_acq``."""

    def desirability_acq(self, program, kind, mean, var, z, best_f=0.0, beta=0.2, alive=None, cross=None, stats=None, form=-1):
        des = from_product(program)
        mu, v = mean.numpy(), var.numpy()
        z = np.ascontiguousarray(z, dtype=np.float64)
        if cross is None:
            self.calls.append(("desirability_q1", kind))
            return self._mask(q1_scores(kind, des, mu, v, z, best_f, beta), alive)
        mp, cpp = stats
        self.calls.append(("desirability_pending", kind))
        out = joint_scores(kind, des, mu, v, cross.numpy(), np.asarray(mp), np.asarray(cpp), z, best_f, beta,
                           None if alive is None else alive.numpy())
        return torch.from_numpy(np.ascontiguousarray(out))


def install(monkeypatch):
    """``_oracle_engine.install`` with ``DesirabilityOracleEngine`` as the engine."""
    import _oracle_engine
    from baybe_amd import engine as engine_mod

    _oracle_engine.install(monkeypatch)
    monkeypatch.setattr(engine_mod, "HipGP", DesirabilityOracleEngine)
    return DesirabilityOracleEngine


# ---- on fitted oracle models, one per target (end-to-end comparisons) ---------------------------------------------------------------
def base_samples(S, q, T, seed):
    return go.sobol_normal_base_samples(S, q * T, seed).reshape(S, q, T)


def model_scores(models, X, pend, des: Des, kind, z, best_f, beta=0.2):
    """Scores of the t-batches [x_i ; pend] under the oracle models' joint posteriors; z [S, q, T]."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    N = len(X)
    if pend is None or len(pend) == 0:
        mv = [m.posterior(X) for m in models]
        return q1_scores(kind, des, np.stack([a for a, _ in mv]), np.stack([b for _, b in mv]), np.asarray(z)[:, 0, :], best_f, beta)
    mu, var, cross, mp, cpp = [], [], [], [], []
    for m in models:
        a, cov = m.posterior_joint(np.vstack([X, pend]))
        mu.append(a[:N]), var.append(np.diag(cov)[:N].copy()), cross.append(cov[:N, N:]), mp.append(a[N:]), cpp.append(cov[N:, N:])
    return joint_scores(kind, des, np.stack(mu), np.stack(var), np.stack(cross), np.stack(mp), np.stack(cpp), z, best_f, beta)


def best_f(models, X_all, des: Des) -> float:
    """max over ALL measurement rows of the desirability of the models' posterior means there."""
    return float(desirability(des, np.stack([m.posterior(X_all)[0] for m in models], axis=-1)).max())


def greedy(models, X, q, seed, des: Des, X_all, kind="qLogEI", S=512, beta=0.2, pending=None):
    """Sequential greedy of ``optimize_acqf_discrete`` (first index on ties, picks leave the candidate set): (indices, values)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    bf = best_f(models, X_all, des)
    base = np.zeros((0, X.shape[1])) if pending is None else np.atleast_2d(pending)
    live = np.ones(len(X), dtype=bool)
    idx, vals = [], []
    for _ in range(q):
        pend = np.vstack([base, X[idx]]) if idx else base
        z = base_samples(S, 1 + len(pend), len(models), seed)
        s = np.where(live, model_scores(models, X, pend, des, kind, z, bf, beta), -np.inf)
        i = int(np.argmax(s))
        idx.append(i), vals.append(float(s[i]))
        live[i] = False
    return idx, vals
