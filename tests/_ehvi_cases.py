"""Cell lists and inputs shared by tests/test_ehvi_cpu.py (which guards the cases) and tests/test_ehvi_gpu.py (which runs them on
the device).

Per-target joint statistics come from ``_joint_cases.JointCase`` through ``_desirability_cases.JointSetData``: one case per target
(seeds of the mean families 0 and 3), target t's rows rolled by t positions, so the regimes of ``_joint_cases.CYCLE`` (ordinary,
jitter 1 / 2 / 3, not-PD, masked) of one row differ between the targets.  The statistics are taken as ORIENTED (every sign + 1; the
orientation is the host's business and is covered end to end).  Cell lists come from fronts of 0 points (one cell, every upper bound
infinite), 1 point and 7 points on a sphere octant (mutually non-dominated) above the reference point -3."""

from __future__ import annotations

import functools

import numpy as np

import _oracle_ehvi as oe
from _desirability_cases import JointSetData
from _joint_cases import JointCase
from oracle import nehvi_oracle as no

FRONT_SIZES = (0, 1, 7)
TARGET_COUNTS = (2, 3, 4)
REF = -3.0


@functools.lru_cache(maxsize=None)
def front(m: int, k: int) -> np.ndarray:
    """k mutually non-dominated points: 2.5 u - 0.5 with u on the positive unit sphere."""
    u = np.abs(np.random.default_rng([m, k]).standard_normal((k, m))) + 0.05
    P = 2.5 * u / np.linalg.norm(u, axis=1, keepdims=True) - 0.5
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def cells(m: int, k: int):
    """(lower [C, m], upper [C, m]) of the front of k points, from the oracle's decomposition."""
    lo, up = no.nondominated_cells(front(m, k), np.full(m, REF))
    lo, up = np.ascontiguousarray(lo), np.ascontiguousarray(up)
    lo.setflags(write=False), up.setflags(write=False)
    return lo, up


# ---- q' = 1 ---------------------------------------------------------------------------------------------------------------------
Q1_SHAPES = [(N, S) for N in (1, 257) for S in (1, 33, 128)]  # S = 33, 128: three and eight sample slices of 16


@functools.lru_cache(maxsize=None)
def q1_inputs(N, S, m):
    """(mean [m, N], var [m, N], z [S, m], alive [N]): at N = 257 rows 3 and 5 need the 1 x 1 jitter in some targets, row 100 is
    masked."""
    from oracle import gp_oracle as go

    rng = np.random.default_rng([N, S, m])
    mean, var = 1.5 * rng.standard_normal((m, N)), 0.05 + 0.5 * rng.random((m, N))
    alive = np.ones(N, dtype=np.uint8)
    if N > 100:
        var[0, 3], var[m - 1, 5], var[1, 5], alive[100] = 0.0, -1e-9, -3e-8, 0
    z = go.sobol_normal_base_samples(S, m, 7).copy()
    for a in (mean, var, z, alive):
        a.setflags(write=False)
    return mean, var, z, alive


# ---- joint ------------------------------------------------------------------------------------------------------------------------
# seeds of the mean families 0 and 3, one per target.  A set that misses a guard of tests/test_ehvi_cpu.py is reseeded HERE (next
# seed of the same family), never loosened on the device.
_SEEDS = (0, 3, 4, 7)
_RESEEDED: dict = {}  # (m, p, target) -> seed


class JointSet:
    """m ``JointCase`` s of the same (p, S, N) stacked target-major, scored against the front of ``k`` points."""

    def __init__(self, m, p, S, N=130, form=0, k=7):
        self.m, self.p, self.S, self.N, self.form, self.k = m, p, S, N, form, k  # form: what ``bbh_ehvi_last_form`` must report
        self.cases = tuple(JointCase(p, S, N, 1.0, _RESEEDED.get((m, p, t), _SEEDS[t])) for t in range(m))
        assert all(c.family in (0, 3) for c in self.cases)

    @property
    def id(self):
        return f"m{self.m}-p{self.p}-S{self.S}-N{self.N}"

    def build(self) -> JointSetData:
        return _build(self.m, self.p, self.S, self.cases)

    def cells(self):
        return cells(self.m, self.k)


@functools.lru_cache(maxsize=None)
def _build(m, p, S, cases):
    return JointSetData(cases, m, p, S)


# N = 130: two full 64-thread workgroups and a ragged one.  form 0: run in the LDS form (asked for by name - left to itself the library
# takes the workspace form, which measured faster); (2, 7): the LDS form at its largest q'; (4, 7): the factors exceed the
# workgroup's share of the LDS, the workspace form.  S = 33: three sample slices (16, 16, 1).
JOINT_SETS = (JointSet(2, 1, 128), JointSet(3, 2, 33), JointSet(4, 3, 33), JointSet(2, 7, 17), JointSet(4, 7, 5, form=1),
              JointSet(3, 2, 33, N=1, k=1))
FORM_SETS = (JointSet(2, 1, 33), JointSet(3, 4, 17))  # both forms legal: bit-for-bit equality


def sigmas(d: JointSetData):
    """[m, N, q, q] joint covariances and [m, N, q] joint means."""
    return np.stack([oe.sigma(d.var[t], d.cross[t], d.cov_pp[t]) for t in range(len(d.mean))]), oe.joint_means(d.mean, d.mean_p)


def compare_rows(got, d: JointSetData, ident: str):
    """NaN rows are exactly the live rows that are notpd in some target, -inf rows exactly the masked rows, every other row is finite."""
    got = np.asarray(got)
    assert np.array_equal(np.isnan(got), d.notpd), (ident, "NaN rows")
    assert np.array_equal(np.isneginf(got), d.masked), (ident, "-inf rows")
    assert np.isfinite(got[d.scored]).all(), (ident, "non-finite score of a live row")


# ---- agreement ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exchangeable_inputs(m: int, p: int, S: int = 33, N: int = 70):
    """(mean [m, N], var [m, N], cross [m, N, p], mean_p [m, p], cov_pp [m, p, p], z [S, p + 1, m]) whose pending points can be
    permuted without changing the draws: per target cross_i = a_i c0, var_i = a_i^2 v00 and cov_pp = D + c0 c0^T / v00 with D
    diagonal, so the Schur complement of the candidate is D for every row and the factor's pending rows are [c0 / sqrt(v00) | sqrt(D)]
    in any order (up to the rounding of the factorisation)."""
    rng = np.random.default_rng([m, p, S, N])
    mean, mean_p = 1.5 * rng.standard_normal((m, N)), 1.5 * rng.standard_normal((m, p))
    a = 0.5 + rng.random((m, N))
    c0, v00, D = 0.3 * rng.standard_normal((m, p)), 0.4 + 0.2 * rng.random(m), 0.1 + 0.5 * rng.random((m, p))
    var = a * a * v00[:, None]
    cross = a[:, :, None] * c0[:, None, :]
    cov_pp = np.stack([np.diag(D[t]) + np.outer(c0[t], c0[t]) / v00[t] for t in range(m)])
    z = oe.base_samples(S, p + 1, m, 13)
    return mean, var, cross, mean_p, cov_pp, z


def permuted(inputs, perm):
    """The same t-batches with the pending points in the order ``perm``."""
    mean, var, cross, mean_p, cov_pp, z = inputs
    perm = np.asarray(perm)
    zp = np.concatenate([z[:, :1, :], z[:, 1 + perm, :]], axis=1)
    return (mean, var, np.ascontiguousarray(cross[:, :, perm]), np.ascontiguousarray(mean_p[:, perm]),
            np.ascontiguousarray(cov_pp[:, perm][:, :, perm]), np.ascontiguousarray(zp))


FAR_BELOW = -1e6  # a pending point there adds nothing: every subset that holds it has an empty (smoothed: e^-70 per target) box


def with_last_far_below(inputs):
    mean, var, cross, mean_p, cov_pp, z = inputs
    mp = mean_p.copy()
    mp[:, -1] = FAR_BELOW
    return mean, var, cross, mp, cov_pp, z


def without_last(inputs):
    """The q' - 1 batch: the last pending point dropped (the leading block of the factor, and the draws of the others, are unchanged)."""
    mean, var, cross, mean_p, cov_pp, z = inputs
    return (mean, var, np.ascontiguousarray(cross[:, :, :-1]), np.ascontiguousarray(mean_p[:, :-1]),
            np.ascontiguousarray(cov_pp[:, :-1, :-1]), np.ascontiguousarray(z[:, :-1, :]))


# ---- through the recommender ---------------------------------------------------------------------------------------------------------
CAMPAIGN_BATCH = 3
CAMPAIGN_PENDING_ROW = 150  # (outside the rows whose values are read back: a candidate that IS a pending point has a singular covariance)
CAMPAIGN_SEED = 1337  # torch.manual_seed before recommend(): the sampler seed is the generator's next draw


def campaign_problem(m: int):
    """(space, measurements, objective, names, signs): 200 candidates in 3 dimensions, 18 measured rows, m targets of which the
    second is minimised (tests/_baybe_shim.py stand-ins)."""
    import pandas as pd

    from _baybe_shim import NumericalTarget, ParetoObjective, SearchSpace

    rng = np.random.default_rng([m, 5])
    cols = ["x0", "x1", "x2"]
    grid = np.round(rng.random((200, 3)), 3)
    grid[0], grid[1] = 0.0, 1.0  # (the parameters' bounds - the surrogates' input scaling - are exactly [0, 1])
    exp = pd.DataFrame(grid, columns=cols)
    space = SearchSpace.from_dataframe(exp)
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), 18, replace=False)].copy()
    X = meas[cols].to_numpy(float)
    f = [-((X - 0.25) ** 2).sum(1), ((X - 0.75) ** 2).sum(1), -np.abs(X - 0.5).sum(1)]
    names = [f"t{j}" for j in range(m)]
    for j, name in enumerate(names):
        meas[name] = f[j] + 0.02 * rng.standard_normal(len(X))
    signs = np.array([1.0, -1.0, 1.0][:m])
    objective = ParetoObjective([NumericalTarget(n, minimize=s < 0) for n, s in zip(names, signs)])
    return space, meas, objective, names, signs


def campaign_ref_point(meas, names, signs):
    """The default reference point: from the oriented measured targets (``compute_ref_point``, factor 0.1)."""
    return no.compute_ref_point(meas[names].to_numpy(float) * signs[None, :])


def next_sampler_seed(seed_value):
    """The seed the next ``draw_sampler_seed`` hands out after ``torch.manual_seed(seed_value)`` (the generator is left there)."""
    import torch

    torch.manual_seed(seed_value)
    s = int(torch.randint(0, 1000000, (1,)).item())
    torch.manual_seed(seed_value)
    return s


def gap_tolerance(log: bool, value: float) -> float:
    """The tolerance the device is held to at a score of this size."""
    from _joint_cases import SCORE_ATOL
    from _objective_cases import MC_ATOL, MC_RTOL

    return SCORE_ATOL if log else MC_ATOL + MC_RTOL * abs(value)
