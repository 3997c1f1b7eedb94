"""Synthetic joint statistics for tests/test_joint_batch_gpu.py (and its CPU guard, tests/test_joint_cases_cpu.py): what the joint
q'-batch acquisition kernels of baybe_amd/csrc/bbh_acq.hip read - candidate mean / variance / cross-covariances, the pending
points' mean and covariance, base samples, best_f, the alive mask - built on the host with known properties, and the oracle's
score of every row.  No GP is involved: ``HipGP.qlogei_pending_big(..., stats=(mean_p, cov_pp))`` takes every statistic from the
caller, so both sides see identical numbers.

A case is (p, S, N, sign, seed).  ``cov_pp = B B^T / (p + 3) + 0.05 I`` is shared by all rows, as on the device.  best_f and the
scale of the covariance belong to a call, not to a row, so the four mean families are a property of the case (``seed % 4``):

  0  means N(0, 1), best_f 0.3
  1  means 0.01 N(0, 1), best_f 0
  2  means 1e-5 N(0, 1), best_f 0, the whole covariance scaled by 1e-10: the objective within a few tau_relu of best_f, near-ties
     between the q' points (rho ~ 1, the sensitive side of the packed quotient)
  3  means 3 N(0, 1), best_f 5: every point far below best_f, tiny fat-softplus values

The rows cycle through the regimes of ``CYCLE``.  With c ~ 0.2 N(0, I) (times the covariance scale) the candidate's variance is
v0 = c^T cov_pp^-1 c + s, s being the Schur complement of the candidate:

  ordinary   s = 1e-3 (times the covariance scale): positive definite as it stands
  jitter k   s = -0.3 h(j_k), j_k = 10^(k-9), where h(j) = j + c^T cov_pp^-1 c - c^T (cov_pp + j I)^-1 c is what a diagonal jitter j
             adds to the Schur complement.  h(j) = j g (1 + O(j / 0.05)) with g = 1 + |cov_pp^-1 c|^2 wherever j is far below the
             eigenvalues of cov_pp (families 0, 1, 3), so there s = -3 10^(k-9) g; in family 2 the jitter is larger than the
             covariance and h(j) ~ j.  Either way h(j_(k-1)) ~ 0.1 h(j_k): the last pivot is -0.2 h(j_k) or below at every smaller
             jitter and +0.7 h(j_k) at j_k - the factorisation fails and succeeds decisively.
  notpd      s = -30 h(1e-6): fails at every level (NaN on the device, LinAlgError in the oracle)
  masked     an ordinary row with alive = 0 (-inf on the device)

Exact duplicates of a pending row are deliberately not used: there the last pivot is +-1e-17 and the level taken is a matter of
rounding, in BoTorch as well."""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

SCORE_ATOL = 1e-8  # the project's tolerance for qLogEI-type scores (tests/test_gpu_parity.py)
JITTERS = (0.0, 1e-8, 1e-7, 1e-6)  # psd_safe_cholesky's ladder, as oracle.gp_oracle._safe_cholesky walks it (1e-8 * 10**attempt)
CYCLE = ("ordinary", "jitter1", "ordinary", "jitter2", "ordinary", "jitter3", "ordinary", "notpd", "ordinary", "jitter1",
         "ordinary", "masked", "ordinary", "jitter2", "jitter3")
# attempts a factorisation of the row takes (the fourth attempt of a notpd row fails as well)
ATTEMPTS = {"ordinary": 1, "masked": 1, "jitter1": 2, "jitter2": 3, "jitter3": 4, "notpd": 4}
# (mean scale, best_f, covariance scale) of the four families
FAMILIES = ((1.0, 0.3, 1.0), (0.01, 0.0, 1.0), (1e-5, 0.0, 1e-10), (3.0, 5.0, 1.0))


@dataclass(frozen=True)
class JointCase:
    p: int
    S: int
    N: int
    sign: float
    seed: int

    @property
    def id(self):
        return f"p{self.p}-S{self.S}-N{self.N}-{'max' if self.sign > 0 else 'min'}-s{self.seed}"

    @property
    def family(self):
        return self.seed % 4

    def build(self):
        return _build(self)

    def reference(self):
        return _reference(self)


@dataclass(frozen=True, eq=False)
class JointData:
    mean: np.ndarray     # [N]
    var: np.ndarray      # [N]
    cross: np.ndarray    # [N, p]
    mean_p: np.ndarray   # [p]
    cov_pp: np.ndarray   # [p, p]
    z: np.ndarray        # [S, p + 1]
    best_f: float
    alive: np.ndarray    # [N] uint8
    labels: tuple        # [N] regime names

    def sigma(self, i):
        """Joint covariance of [candidate i ; pending], candidate first."""
        p = len(self.mean_p)
        A = np.empty((p + 1, p + 1))
        A[0, 0] = self.var[i]
        A[0, 1:] = A[1:, 0] = self.cross[i]
        A[1:, 1:] = self.cov_pp
        return A

    def joint_mean(self, i):
        return np.concatenate([self.mean[i:i + 1], self.mean_p])

    def is_label(self, *names):
        return np.array([lab in names for lab in self.labels])

    @property
    def scored(self):
        """Live rows with a factor: the rows whose score is a number."""
        return ~self.is_label("masked", "notpd")


@functools.lru_cache(maxsize=None)
def _build(case: JointCase) -> JointData:
    from oracle import gp_oracle as go

    p, S, N = case.p, case.S, case.N
    mscale, best_f, cscale = FAMILIES[case.family]
    rng = np.random.default_rng([p, S, N, int(case.sign < 0), case.seed])
    B = rng.standard_normal((p, p + 3))
    cov_pp = (B @ B.T / (p + 3) + 0.05 * np.eye(p)) * cscale
    cov_pp = 0.5 * (cov_pp + cov_pp.T)
    cross = 0.2 * cscale * rng.standard_normal((N, p))
    mean = mscale * rng.standard_normal(N)
    mean_p = mscale * rng.standard_normal(p)
    labels = tuple(CYCLE[i % len(CYCLE)] for i in range(N))
    # in the eigenbasis of cov_pp: c^T cov_pp^-1 c = sum ct^2 / lam, h(j) - j = sum ct^2 j / (lam (lam + j)) without cancellation
    lam, V = np.linalg.eigh(cov_pp)
    ct2 = (cross @ V) ** 2
    quad = (ct2 / lam).sum(axis=1)

    def h(j):
        return j + (ct2 * (j / (lam * (lam + j)))).sum(axis=1)

    s = np.full(N, 1e-3 * cscale)
    for k in (1, 2, 3):
        rows = np.array([lab == f"jitter{k}" for lab in labels])
        s[rows] = -0.3 * h(JITTERS[k])[rows]
    rows = np.array([lab == "notpd" for lab in labels])
    s[rows] = -30.0 * h(JITTERS[3])[rows]
    alive = np.array([lab != "masked" for lab in labels], dtype=np.uint8)
    z = go.sobol_normal_base_samples(S, p + 1, case.seed)
    out = JointData(mean, quad + s, cross, mean_p, cov_pp, z, best_f, alive, labels)
    for a in (out.mean, out.var, out.cross, out.mean_p, out.cov_pp, out.z, out.alive):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(case: JointCase) -> np.ndarray:
    """The oracle's score of every row (``qlogei_joint``, row by row): -inf for masked rows, NaN where it raises LinAlgError.
    Computed once per case and shared (read-only)."""
    import scipy.linalg as sla

    from oracle import gp_oracle as go

    d = case.build()
    out = np.empty(case.N)
    for i in range(case.N):
        if not d.alive[i]:
            out[i] = -np.inf
            continue
        try:
            out[i] = go.qlogei_joint(d.joint_mean(i), d.sigma(i), d.z, d.best_f, case.sign)
        except sla.LinAlgError:
            out[i] = np.nan
    out.setflags(write=False)
    return out


# ---- the case tables of tests/test_joint_batch_gpu.py --------------------------------------------------
N_ROWS = 777  # three full 256-thread workgroups and a ragged one; twelve 64-thread ones and a ragged one
REGISTER_S = (33, 100, 512)  # at 777 rows the default handle takes 1, 3 (34 / 34 / 32 samples) and 16 sample slices


# Seeds are replaced by the next one of the same family where the draw misses a condition of tests/test_joint_cases_cpu.py:
# (b) a wrong jitter level nearly invisible - mostly the family far below best_f, where the score hardly depends on the degenerate
#     direction;
# (e) a reference that its own rounding does not resolve - a jitter row of that family whose near-singular pivot comes before the last
#     row of the factor, with one sample just above best_f carrying the whole score (p = 3, S = 512: 2e-7 under a 4 ulp perturbation
#     of the covariance; the device's LDS and register forms both stood 1.6e-8 from LAPACK's factor there, the kernels' loop restated
#     in numpy 1e-9).  Seeds within a factor of four of that bound are replaced as well.
RESEEDED = {(2, 512, -1.0, 7): 11, (7, 512, 1.0, 11): 15, (10, 33, -1.0, 11): 15, (10, 100, 1.0, 12): 16, (10, 512, -1.0, 15): 23,
            (15, 128, 1.0, 3): 19, (3, 512, 1.0, 7): 11, (4, 100, -1.0, 7): 15, (5, 100, 1.0, 7): 15, (7, 33, 1.0, 7): 11}


def _case(p, S, N, sign, seed):
    return JointCase(p, S, N, sign, RESEEDED.get((p, S, sign, seed), seed))


def register_cases(p):
    """p = 1 ... 13 (Q = 2 ... 14): every S and sign; the seeds walk the four families for every p, S and sign."""
    return [_case(p, S, N_ROWS, sign, p + 2 * a + b) for a, S in enumerate(REGISTER_S) for b, sign in enumerate((1.0, -1.0))]


REGISTER_P = tuple(range(1, 14))
ONE_ROW_CASE = JointCase(5, 100, 1, 1.0, 0)
# q' = 15, 16: the LDS form whatever the sample count
LDS_CASES = (JointCase(14, 33, N_ROWS, 1.0, 0), JointCase(14, 128, N_ROWS, -1.0, 1), JointCase(15, 33, N_ROWS, -1.0, 2),
             _case(15, 128, N_ROWS, 1.0, 3))
# 8 (S q' + p + p^2) bytes against 60 KB at q' = 14: 61 376 B (register form, its largest dynamic-LDS launch with one slice) and
# 61 488 B (LDS form); 66 008 B at S = 1024, q' = 8 (LDS form)
HANDOVER_CASES = (JointCase(13, 535, N_ROWS, 1.0, 4), JointCase(13, 536, N_ROWS, -1.0, 5))
S1024_CASE = JointCase(7, 1024, N_ROWS, 1.0, 2)
LDS_SWITCH_P = (1, 6, 13)  # Q = 2, 7, 14 under BBH_PENDING_LDS=1


def lds_switch_cases(p):
    return [c for c in register_cases(p) if c.S in (33, 100)]


# q' > 16: the factor in a global workspace (BBH_QBIG_WS_MB=1: 300 rows are one chunk at q' = 17, two at 33, five at 64)
BIG_CASES = (JointCase(16, 64, 300, 1.0, 0), JointCase(16, 64, 300, -1.0, 3), JointCase(32, 64, 300, -1.0, 1),
             JointCase(63, 64, 300, 1.0, 2))


def form_bytes(case):
    """What ``bbh_qlogei_pending_impl`` holds against 60 KB to choose between the register and the LDS form."""
    return 8 * (case.S * (case.p + 1) + case.p + case.p * case.p)


def all_cases():
    out = [c for p in REGISTER_P for c in register_cases(p)]
    out += [ONE_ROW_CASE, *LDS_CASES, *HANDOVER_CASES, S1024_CASE, *BIG_CASES]
    return out


# ---- the checks both test modules share ---------------------------------------------------------------
def compare(got: np.ndarray, case: JointCase, ref: np.ndarray | None = None) -> float:
    """NaN rows are exactly the notpd rows, -inf rows exactly the masked rows; the largest |score - reference| over the others."""
    d = case.build()
    ref = case.reference() if ref is None else ref
    got = np.asarray(got)
    assert got.shape == ref.shape, (case.id, got.shape)
    assert np.array_equal(np.isnan(got), d.is_label("notpd")), (case.id, "NaN rows", np.nonzero(np.isnan(got) != d.is_label("notpd"))[0][:10])
    assert np.array_equal(np.isneginf(got), d.is_label("masked")), (case.id, "-inf rows", np.nonzero(np.isneginf(got) != d.is_label("masked"))[0][:10])
    live = d.scored
    assert np.isfinite(got[live]).all(), (case.id, "non-finite score of a live row")
    return float(np.abs(got[live] - ref[live]).max()) if live.any() else 0.0


# ---- CPU-side restatements (tests/test_joint_cases_cpu.py) ---------------------------------------------
def lapack_attempts(A: np.ndarray):
    """(attempts, succeeded) of ``oracle.gp_oracle._safe_cholesky`` on A: the level it took is read off L L^T - A."""
    import scipy.linalg as sla

    from oracle import gp_oracle as go

    try:
        L = go._safe_cholesky(A)
    except sla.LinAlgError:
        return 4, False
    taken = float(np.mean(np.diag(L @ L.T - A)))
    level = int(np.argmin([abs(taken - j) for j in JITTERS]))
    assert abs(taken - JITTERS[level]) <= 1e-3 * max(JITTERS[level], 1e-12) + 1e-14 * np.abs(A).max(), (taken, level)
    return level + 1, True


def unblocked_attempts(Sig: np.ndarray):
    """The kernels' factorisation - row by row, a pivot ``not (s > 0)`` ends the attempt, then the next jitter - on a stack
    Sig [N, q, q] at once.  Returns (attempts [N], succeeded [N], deciding [N]): the smallest magnitude among the pivots that decided
    an attempt of the row - the failing pivot of every failed attempt, the smallest pivot of the successful one."""
    N, q, _ = Sig.shape
    attempts = np.zeros(N, dtype=int)
    done = np.zeros(N, dtype=bool)
    deciding = np.full(N, np.inf)
    for a, jit in enumerate(JITTERS):
        L = np.zeros_like(Sig)
        failed = np.zeros(N, dtype=bool)
        fail_pivot = np.zeros(N)
        min_pivot = np.full(N, np.inf)
        with np.errstate(invalid="ignore", divide="ignore"):
            for r in range(q):
                for c in range(r + 1):
                    s = Sig[:, r, c] + (jit if r == c else 0.0)
                    for k in range(c):
                        s = s - L[:, r, k] * L[:, c, k]
                    if r == c:
                        bad = ~failed & ~(s > 0.0)
                        fail_pivot[bad] = s[bad]
                        failed |= bad
                        min_pivot = np.where(failed, min_pivot, np.minimum(min_pivot, s))
                        L[:, r, r] = np.sqrt(np.where(s > 0.0, s, np.nan))
                    else:
                        L[:, r, c] = s / L[:, c, c]
        todo = ~done
        attempts[todo] = a + 1
        decided = np.where(failed, np.abs(fail_pivot), min_pivot)
        deciding[todo] = np.minimum(deciding[todo], decided[todo])
        done |= ~failed
    return attempts, done, deciding


def dense_score(mean: np.ndarray, cov: np.ndarray, jitter: float, z: np.ndarray, best_f: float, sign: float) -> float:
    """qLogEI of one q'-batch restated without the oracle: Cholesky of cov + jitter I, then log-fat-softplus, fat maximum and
    log-mean-exp of the full [S, q'] matrix (botorch.utils.safe_math, botorch.acquisition.logei)."""
    import scipy.linalg as sla
    from scipy.special import logsumexp

    tau_relu, tau_max = 1e-6, 1e-2
    L = sla.cholesky(cov + jitter * np.eye(len(mean)), lower=True)
    t = (sign * (mean[None, :] + z @ L.T) - best_f) / tau_relu
    li = np.log(tau_relu) + np.log(np.logaddexp(0.0, t) + 0.1 / (1.0 + t * t))
    M = li.max(axis=1)
    fm = M + tau_max * np.log(((2.0 / (2.0 + (M[:, None] - li) / tau_max)) ** 2).sum(axis=1))
    return float(logsumexp(fm) - np.log(len(fm)))
