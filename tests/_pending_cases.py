"""Models, pending sets, candidates and oracle references for tests/test_pending_passes_gpu.py (and its CPU guard,
tests/test_pending_cases_cpu.py): the passes that produce the ``cross`` input of the joint q'-batch acquisition kernels - the mean-only
pass of the fused posterior kernel (``cross_cov``), the variance pass while pending points are set, ``bbh_coopg_cross_kernel``, the
materialised-K* and feature-space paths - and the handle's pending state behind them.

A model (``PendModel``) is a kernel, d numerical columns, n training rows, optionally an ICM table over T tasks or an outputscale, and
a column layout; its data comes from ``_problems.make_problem`` / ``make_tl_problem``, its hyper-parameters are ``fixed_theta(d)``
(noise e^-5) with per-column lengthscales jittered by [0.8, 1.2].  A case (``PendCase``) adds p pending points and N candidate rows.

Pending point j is, by j mod 3: a grid row outside the training set, a training row, a row 1e-3 (unit cube) from a training row; in a
task model it lies in task (j + 1) mod T.  The candidate set is always built for 257 rows and cut to N, so a shorter launch scores a
prefix of the longer one.  Rows 0 .. 10 and 246 .. 256 are special (``CaseData.labels``):

  pending:j   the row IS pending point j (task included): its cross column j is the posterior variance of that point
  train:k     the row is training row k
  near:j      pending point j moved by 1e-3 in every unit coordinate
  corner      all ones / all zeros in the unit cube, far from the data

and every other row is a grid row in task i mod T.  Row 256 is ``pending:p-1``: alone in the seventeenth tile.

The reference is the oracle, batched as ``tests/_oracle_engine.py::cross_cov`` (``reference``); deviations are scaled and absolute
(``scaled_cross`` / ``scaled_var`` / ``scaled_mean``), held to ``TOL`` = 1e-11.  ``longdouble_reference`` restates the same formulas
in ``np.longdouble`` - kernel values, column Cholesky, forward substitution - and the CPU guard requires the float64 oracle to be
within ``REF_NOISE`` = 1e-13 of it for every case.

THE TABLE OF FAMILY A (every instantiation of ``bbh_fused_launch_kd*``; read off ``bbh_launch_fused``: kd = ceil((d + 2) / 4) rounded
up to 2 / 4 / 6 / 8 / 12 / 16, the pipelined form for Matérn-5/2 with or without a table and for RBF / Matérn-3/2 without, the plain
form - ``bbh_fused_launch_kd0`` - for everything else, for kd > 16 and under BBH_PIPELINE=0):

  KD  d   Matérn-5/2            Matérn-5/2 + table            RBF                   Matérn-3/2
  2   3   n 1 p 15, n 16 p 1    scale n 15 p 15, n 64 p 2     n 17 p 15, n 300 p 8  n 65 p 15, n 17 p 1
  4   9   n 300 p 15, n 65 p 2  ICM n 1 p 15, n 15 p 8        n 15 p 15, n 16 p 1   n 17 p 15, n 16 p 2
  6   20  n 65 p 15, n 64 p 8   ICM n 300 p 15, n 17 p 8      n 1 p 15, n 17 p 2    n 15 p 15, n 65 p 8
  8   28  n 17 p 15, n 1 p 1    scale n 65 p 15, n 15 p 2     n 300 p 15, n 16 p 8  n 1 p 15, n 64 p 1
  12  40  n 15 p 15, n 300 p 2  scale n 17 p 15, n 65 p 8     n 65 p 15, n 1 p 1    n 300 p 15, n 1 p 2
  16  62  n 1 p 15, n 15 p 8    scale n 15 p 15, n 16 p 1     n 17 p 15, n 64 p 2   n 65 p 15, n 300 p 8
  6   20  Matérn-5/2, n 513: p 15 and p 2 (nb_ext = 37)
  ("scale": a ScaleKernel without tasks - a table of one entry; "ICM": a 4-task table, pending points in three or four tasks)
  plain    Matérn-5/2 d 70 (kd 18): n 17 p15, n 64 p2;  Matérn-5/2 + scale d 70: n 15 p15;  Matérn-1/2 d 9: n 15 p15, n 65 p1;
           RBF + ICM d 9: n 17 p15;  Matérn-3/2 + scale d 3: n 65 p8
  BBH_PIPELINE=0 (plain form at small d): Matérn-5/2 d 3 n 17 p15; Matérn-5/2 + ICM d 9 n 15 p15; RBF d 20 n 65 p15;
           Matérn-3/2 d 3 n 1 p15

(``family_a()`` builds it; ``test_pending_cases_cpu.py::test_family_a_covers_every_instantiation`` holds it to the rule: every
instantiation with an n that is no multiple of 16 and p = 15.)"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from _problems import fixed_theta, make_problem, make_tl_problem, oracle_params, oracle_spec

TOL = 1e-11        # device against the oracle, scaled (tests/test_gpu_parity.py::test_pipelined_kernel_matches_plain_form)
REF_NOISE = 1e-13  # float64 oracle against its long-double restatement, scaled
PEND_MEAN_ATOL = 1e-10  # ``set_pending`` means, in units of ysd
N_FULL = 257       # four full 64-candidate workgroups and one row: sixteen full tiles and a ragged one
LD = np.longdouble

KD_DIMS = {2: 3, 4: 9, 6: 20, 8: 28, 12: 40, 16: 62}
GENERIC = ("product", "scaled_sum", "three", "sum3", "nested4", "product4", "rq", "piecewise2", "linear", "poly2", "periodic",
           "product_m12", "matern_x_poly2", "linear_plus_rbf", "nested_dot", "rq_first3", "rq_second")


@dataclass(frozen=True)
class PendModel:
    kernel: str            # "matern52" | "matern32" | "matern12" | "rbf" | one of GENERIC | "rff16" | "rff64"
    d: int                 # numerical columns
    n: int
    tasks: int = 0         # T > 1: an ICM table over T tasks (one more column)
    scale: bool = False    # ScaleKernel around a single kernel (a table without tasks)
    layout: str = "unit"   # "unit": columns in [0, 1], task column last; "mixed": non-unit lo / hi, task column in the middle
    seed: int = 0
    noise: float = 0.0         # > 0: the noise variance instead of ``fixed_theta``'s e^-5 (RFF: 0.05)
    ls_scale: float = 1.0      # multiplies the lengthscales of every distance factor (Matérn, RBF, RQ)
    rq_ls_scale: float = 1.0   # ... and those of the RQ factors alone
    rq_alpha: float = 0.0      # > 0: alpha of the RQ factors instead of 0.8

    @property
    def id(self):
        return (f"{self.kernel}-d{self.d}-n{self.n}" + (f"-T{self.tasks}" if self.tasks else "") + ("-scale" if self.scale else "")
                + ("-mixed" if self.layout == "mixed" else "") + (f"-s{self.seed}" if self.seed else "")
                + (f"-nz{self.noise:g}" if self.noise else "") + (f"-ls{self.ls_scale:.3g}" if self.ls_scale != 1.0 else "")
                + (f"-rqls{self.rq_ls_scale:.3g}" if self.rq_ls_scale != 1.0 else "") + (f"-a{self.rq_alpha:g}" if self.rq_alpha else ""))

    @property
    def generic(self):
        return self.kernel in GENERIC

    @property
    def rff(self):
        return self.kernel.startswith("rff")

    @property
    def dtot(self):
        return self.d + (1 if self.tasks else 0)

    @property
    def task_col(self):
        return None if not self.tasks else (self.d // 2 if self.layout == "mixed" else self.d)

    @property
    def nb(self):
        """Training column blocks of 16: n is padded to a multiple of 64."""
        return 4 * ((self.n + 63) // 64)

    @property
    def pass_widths(self):
        """Windows of the variance pass: 16 blocks wide, the remainder last (``bbh_pack_operands``)."""
        full, rest = divmod(self.nb, 16)
        return (16,) * full + ((rest,) if rest else ())

    @property
    def kd(self):
        """k-steps of the distance GEMM (``bbh_set_model``): rounded up to an instantiated count, 18 and more as they are."""
        kd = (self.d + 5) // 4
        for c in (2, 4, 6, 8, 12, 16):
            if kd <= c:
                return c
        return kd

    @property
    def has_tbl(self):
        return self.tasks > 1 or self.scale

    def windowed_instantiation(self, pipeline=True):
        """Which ``bbh_fused_posterior_kernel`` instantiation the windowed form runs this model as: (KD, kind, table) with KD = 0
        for the plain form (``kdp`` in ``bbh_launch_fused``)."""
        assert not self.generic and not self.rff
        m52 = self.kernel == "matern52"
        piped = (m52 or (self.kernel in ("rbf", "matern32") and not self.has_tbl)) and pipeline and self.kd <= 16
        if piped:
            return self.kd, self.kernel, self.has_tbl
        return 0, ("matern52" if m52 else "runtime"), self.has_tbl

    def build(self):
        return _build_model(self)


@dataclass(frozen=True)
class PendCase:
    family: str
    model: PendModel
    p: int
    N: int = N_FULL
    handle: str = "default"   # the switches of the handle the GPU test runs it on (tests/test_pending_passes_gpu.py::VARIANTS)
    pend_seed: int = 0

    @property
    def id(self):
        return (f"{self.family}-{self.model.id}-p{self.p}-N{self.N}" + (f"-{self.handle}" if self.handle != "default" else "")
                + (f"-ps{self.pend_seed}" if self.pend_seed else ""))

    @property
    def key(self):
        """What the data and the reference depend on (not the family, not the handle)."""
        return self.model, self.p, self.N, self.pend_seed

    def build(self):
        return _build_case(*self.key)

    def reference(self):
        return _reference(*self.key)


# ---- models ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class ModelData:
    spec: object        # baybe_amd.gp_spec.GPSpec
    params: object      # baybe_amd.gp_spec.GPParams
    Xt: np.ndarray      # [n, dtot] raw training rows
    y: np.ndarray
    Ut: np.ndarray      # [n, d] unit-cube coordinates of the training rows
    tt: np.ndarray      # [n] their tasks
    pool: np.ndarray    # [*, d] unit-cube grid rows outside the training set
    lo: np.ndarray      # [d] bounds of the numerical columns
    hi: np.ndarray
    om: object          # oracle.gp_oracle.GPModel

    def assemble(self, model: PendModel, U: np.ndarray, t: np.ndarray) -> np.ndarray:
        """Raw rows [*, dtot] of unit-cube coordinates U and tasks t in the model's column layout."""
        out = np.empty((len(U), model.dtot))
        num = [c for c in range(model.dtot) if c != model.task_col]
        out[:, num] = self.lo + (self.hi - self.lo) * U
        if model.tasks:
            out[:, model.task_col] = t
        return np.ascontiguousarray(out)


def _generic_kernel(name):
    from baybe_amd.kernels import (AdditiveKernel, LinearKernel, MaternKernel, PeriodicKernel, PiecewisePolynomialKernel,
                                   PolynomialKernel, ProductKernel, RBFKernel, RQKernel, ScaleKernel)

    return {
        "product": ProductKernel([MaternKernel(2.5), ScaleKernel(RBFKernel())]),
        "scaled_sum": AdditiveKernel([ScaleKernel(MaternKernel(1.5)), ScaleKernel(RBFKernel())]),
        "three": ProductKernel([RBFKernel(), MaternKernel(1.5), ScaleKernel(MaternKernel(2.5))]),
        "sum3": AdditiveKernel([ScaleKernel(MaternKernel(2.5)), ScaleKernel(RBFKernel()), ScaleKernel(RQKernel())]),
        # the nested entry of the reference's kernel matrix: (Matern * Matern) + (Matern + RBF)
        "nested4": AdditiveKernel([ProductKernel([MaternKernel(2.5), MaternKernel(1.5)]),
                                   AdditiveKernel([ScaleKernel(MaternKernel(2.5)), RBFKernel()])]),
        "product4": ProductKernel([RBFKernel(), MaternKernel(1.5), MaternKernel(2.5), ScaleKernel(RQKernel())]),
        "rq": ScaleKernel(RQKernel()),
        "piecewise2": ScaleKernel(PiecewisePolynomialKernel(2)),
        "linear": ScaleKernel(LinearKernel()),
        "poly2": ScaleKernel(PolynomialKernel(2)),
        "periodic": ScaleKernel(PeriodicKernel()),
        "product_m12": ProductKernel([MaternKernel(0.5), ScaleKernel(RBFKernel())]),  # a Matérn-1/2 factor: materialised K* only
        # dot kinds inside a composition (a per-candidate k(x, x)), the grouped combine with a dot kind and a periodic factor, RQ as
        # the first and as a later factor (tests/_generic_variance_cases.py)
        "matern_x_poly2": ProductKernel([MaternKernel(2.5), ScaleKernel(PolynomialKernel(2))]),
        "linear_plus_rbf": AdditiveKernel([ScaleKernel(LinearKernel()), ScaleKernel(RBFKernel())]),
        "nested_dot": AdditiveKernel([ProductKernel([MaternKernel(2.5), LinearKernel()]),
                                      AdditiveKernel([ScaleKernel(RBFKernel()), ScaleKernel(PeriodicKernel())])]),
        "rq_first3": ProductKernel([RQKernel(), MaternKernel(2.5), ScaleKernel(RBFKernel())]),
        "rq_second": ProductKernel([MaternKernel(2.5), ScaleKernel(RQKernel())]),
    }[name]


def _make_spec(model: PendModel, lo_full, hi_full):
    from baybe_amd import gp_spec
    from baybe_amd.kernels import RFFKernel, ScaleKernel, apply_kernel_spec

    kw = dict(task_idx=model.task_col, n_tasks=model.tasks) if model.tasks else {}
    if model.generic or model.rff:
        spec = gp_spec.GPSpec.baybe_default(model.dtot, lo_full, hi_full, **kw)
        kern = ScaleKernel(RFFKernel(int(model.kernel[3:]))) if model.rff else _generic_kernel(model.kernel)
        apply_kernel_spec(spec, kern)
        if model.rff:  # the frequencies belong to the model: fixed here, so that both sides and every handle hold the same ones
            spec.rff_weights = np.random.default_rng(1000 + model.seed).standard_normal((model.d, spec.rff_num_samples))
    else:
        spec = gp_spec.GPSpec.baybe_default(model.dtot, lo_full, hi_full, kernel=model.kernel, **kw)
        spec.use_outputscale = bool(model.scale)
    return spec


def _make_params(model: PendModel, spec, rng):
    """``fixed_theta(d)`` with jittered lengthscales; the members of the generic family by kind: Linear variances 1.5 / d, the
    Polynomial offset 1.5 on inputs in [0, 1]^d (its weights are pinned to 1), periods near 1.3, RQ alpha 0.8, a piecewise support of
    several cube diagonals - values at which every case meets the reference-noise condition (tests/test_pending_cases_cpu.py)."""
    from baybe_amd import gp_spec

    d = model.d
    ls0, nz, _ = fixed_theta(d)
    p = gp_spec.initial_params(spec)
    jit = lambda: 0.8 + 0.4 * rng.random(d)  # noqa: E731
    kinds = spec.factor_kinds
    F = len(kinds)

    def ls_of(kind):
        if kind == "linear":
            return (1.5 / d) ** -0.5 * jit()  # the weights w = v^-1/2
        if kind.startswith("poly"):
            return np.ones(d)
        if kind == "periodic":
            return 1.5 * jit()
        if kind.startswith("piecewise"):
            return 4.0 * math.sqrt(d) * jit()
        out = ls0 * (math.sqrt(F) if F > 1 and spec.combine == "product" else 1.0) * jit()
        if model.ls_scale != 1.0:
            out = out * model.ls_scale
        if kind == "rq" and model.rq_ls_scale != 1.0:
            out = out * model.rq_ls_scale
        return out

    p.lengthscale = ls_of(kinds[0])
    if F > 1:
        p.factor_ls = [ls_of(k) for k in kinds[1:]]
        p.factor_os = np.where(np.array([f.scaled for f in spec.factors]), 0.6 + 0.8 * rng.random(F), 1.0)
    if spec.has_rq:
        p.alpha = np.array([(model.rq_alpha or 0.8) if k == "rq" else (1.5 if k.startswith("poly") else 1.0) for k in kinds])
    if spec.has_periodic:
        p.period = [(1.3 * jit()) if k == "periodic" else np.ones(d) for k in kinds]
    p.noise, p.mean = model.noise or (0.05 if model.rff else nz), 0.03  # (a rank-2D kernel: at e^-5 the oracle's own mean is 2e-13 from its restatement)
    if spec.use_outputscale:  # (a Polynomial kernel is (d / 3 + offset)^2 at a typical row: scaled back to the order of 1)
        p.outputscale = 1.7 / (d / 3.0 + 1.5) ** 2 if model.kernel == "poly2" else 1.7
    if model.tasks:
        T = model.tasks
        p.task_W = 0.3 + rng.random((T, T))
        p.task_v = 0.5 + rng.random(T)
    return p


@functools.lru_cache(maxsize=None)
def _build_model(model: PendModel) -> ModelData:
    from oracle import gp_oracle as go

    d, n, T = model.d, model.n, model.tasks
    rng = np.random.default_rng([17, d, n, T, model.seed, int(model.scale), sum(map(ord, model.kernel))])
    if T:
        per = (n + T - 1) // T
        X, rows, y = make_tl_problem(n + 700, d, per, T=T, seed=model.seed + 3)
        keep = np.sort(rng.permutation(len(rows))[:n])  # n need not be a multiple of T
        Ut, tt, y = rows[keep, :d], rows[keep, d].astype(np.int64), y[keep]
        grid = X[:, :d]
    else:
        grid, Ut, y = make_problem(n + 700, d, n, seed=model.seed + 3)
        tt = np.zeros(n, dtype=np.int64)
    seen = {r.tobytes() for r in np.ascontiguousarray(Ut)}
    uniq = []
    for r in np.ascontiguousarray(grid):  # distinct grid rows outside the training set, in the grid's order
        k = r.tobytes()
        if k not in seen:
            seen.add(k)
            uniq.append(r)
    pool = np.array(uniq)
    assert len(pool) >= N_FULL + 64, (model.id, len(pool))
    if model.layout == "mixed":
        lo, hi = -0.5 - 0.1 * np.arange(d), 1.5 + 0.2 * np.arange(d)
    else:
        lo, hi = np.zeros(d), np.ones(d)
    lo_full, hi_full = np.zeros(model.dtot), np.ones(model.dtot)
    num = [c for c in range(model.dtot) if c != model.task_col]
    lo_full[num], hi_full[num] = lo, hi
    spec = _make_spec(model, lo_full, hi_full)
    params = _make_params(model, spec, rng)
    md = ModelData(spec, params, None, y, Ut, tt, pool, lo, hi, None)
    Xt = md.assemble(model, Ut, tt)
    om = go.GPModel(oracle_spec(spec), oracle_params(spec, params), Xt, y)
    assert om.jitter == 0.0, model.id
    md = ModelData(spec, params, Xt, y, Ut, tt, pool, lo, hi, om)
    for a in (md.Xt, md.y, md.Ut, md.tt, md.pool):
        a.setflags(write=False)
    return md


# ---- cases ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class CaseData:
    cand: np.ndarray    # [N, dtot] raw candidate rows
    P: np.ndarray       # [p, dtot] raw pending points
    labels: tuple       # [N]
    Uc: np.ndarray      # unit-cube coordinates / tasks behind them (the injected defects of the CPU guard rebuild rows from these)
    tc: np.ndarray
    Up: np.ndarray
    tp: np.ndarray

    def rows(self, prefix):
        return np.array([lab.startswith(prefix) for lab in self.labels])


def pending_points(model: PendModel, p: int, pend_seed: int = 0):
    """(unit coordinates [p, d], tasks [p]) of the pending set: by j mod 3 a grid row outside the training set and outside the
    candidate rows, a training row, a row 1e-3 from a training row."""
    md = model.build()
    n, T = model.n, model.tasks
    U, t = np.empty((p, model.d)), np.zeros(p, dtype=np.int64)
    for j in range(p):
        k = (j // 3 + 5 * pend_seed) % n
        fresh = md.pool[N_FULL + 16 * pend_seed + j]
        if j % 3 == 1 and j // 3 < n:
            U[j] = md.Ut[k]
        elif j % 3 == 2 and j // 3 < n:
            U[j] = md.Ut[k] + 1e-3 * (1 + j // 3)
        else:
            U[j] = fresh
        t[j] = (j + 1 + pend_seed) % T if T else 0
    return U, t


@functools.lru_cache(maxsize=None)
def _build_case(model: PendModel, p: int, N: int, pend_seed: int) -> CaseData:
    md = model.build()
    T = model.tasks
    Up, tp = pending_points(model, p, pend_seed)
    Uc = md.pool[:N_FULL].copy()
    tc = (np.arange(N_FULL) % T) if T else np.zeros(N_FULL, dtype=np.int64)
    labels = ["ordinary"] * N_FULL
    special = []
    if p:
        special += [("pending", j) for j in sorted({0, p // 2, p - 1})]
    special += [("train", k) for k in sorted({0, model.n // 2, model.n - 1})]
    if p:
        special += [("near", j) for j in sorted({0, p - 1})]
    special += [("corner", 1), ("corner", 0)]
    tail = ([("near", 0)] if p else []) + [("train", model.n - 1), ("corner", 1)] + ([("pending", 0), ("pending", p - 1)] if p else [])
    for i, (what, k) in list(enumerate(special)) + [(N_FULL - len(tail) + a, s) for a, s in enumerate(tail)]:
        if what == "pending":
            Uc[i], tc[i] = Up[k], tp[k]
        elif what == "train":
            Uc[i], tc[i] = md.Ut[k], md.tt[k]
        elif what == "near":
            Uc[i], tc[i] = Up[k] + 1e-3, tp[k]
        else:  # (a Linear kernel has k(0, 0) = 0, where no scaled deviation is defined: both corners are the far one)
            Uc[i] = 1.0 if model.kernel == "linear" else float(k)
        labels[i] = "corner" if what == "corner" else f"{what}:{k}"
    out = CaseData(md.assemble(model, Uc, tc)[:N], md.assemble(model, Up, tp) if p else np.empty((0, model.dtot)), tuple(labels[:N]),
                   Uc[:N], tc[:N], Up, tp)
    for a in (out.cand, out.P, out.Uc, out.tc, out.Up, out.tp):
        a.setflags(write=False)
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Reference:
    mean: np.ndarray     # [N]
    var: np.ndarray      # [N]
    cross: np.ndarray    # [N, p]
    mean_p: np.ndarray   # [p]
    cov_pp: np.ndarray   # [p, p]
    kxx: np.ndarray      # [N] prior variances of the candidates (outputscale and task factor included), standardised scale
    kpp: np.ndarray      # [p]
    ysd: float


def batched_cross(om, cand, P):
    """``tests/_oracle_engine.py::OracleEngine.cross_cov``: cross = ysd^2 (K(X*, P) - Vc^T Vp), V = L^-1 K(., X)^T."""
    import scipy.linalg as sla

    from oracle import gp_oracle as go

    Xcn, Pn = go.normalize_inputs(om.spec, cand), go.normalize_inputs(om.spec, P)
    Vc = sla.solve_triangular(om.L, go.cross_cov(om.spec, om.params, Xcn, om.Xn).T, lower=True)
    Vp = sla.solve_triangular(om.L, go.cross_cov(om.spec, om.params, Pn, om.Xn).T, lower=True)
    return om.ysd**2 * (go.cross_cov(om.spec, om.params, Xcn, Pn) - Vc.T @ Vp)


@functools.lru_cache(maxsize=None)
def _reference(model: PendModel, p: int, N: int, pend_seed: int) -> Reference:
    return reference_of(model, _build_case(model, p, N, pend_seed))


def reference_of(model: PendModel, d: CaseData) -> Reference:
    """The oracle's posterior of the rows ``d.cand`` and their cross-covariances with the pending points ``d.P``."""
    from oracle import gp_oracle as go

    om = model.build().om
    p, N = len(d.P), len(d.cand)
    mean, var = om.posterior(d.cand)
    kxx = go.prior_var(om.spec, om.params, go.normalize_inputs(om.spec, d.cand))
    if p:
        cross = batched_cross(om, d.cand, d.P)
        mean_p, cov_pp = om.posterior_joint(d.P)
        kpp = go.prior_var(om.spec, om.params, go.normalize_inputs(om.spec, d.P))
    else:
        cross, mean_p, cov_pp, kpp = np.empty((N, 0)), np.empty(0), np.empty((0, 0)), np.empty(0)
    out = Reference(mean, var, cross, mean_p, cov_pp, kxx, kpp, float(om.ysd))
    for a in (out.mean, out.var, out.cross, out.mean_p, out.cov_pp, out.kxx, out.kpp):
        a.setflags(write=False)
    return out


def scaled_cross(got, ref: Reference, want=None) -> float:
    """max |got - ref| / (ysd^2 sqrt(k(x, x) k(p_j, p_j))) over all rows and columns."""
    want = ref.cross if want is None else want
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not got.size:
        return 0.0
    dev = np.abs(got - want) / (ref.ysd**2 * np.sqrt(ref.kxx[:, None] * ref.kpp[None, :]))
    return float(dev.max()) if np.isfinite(got).all() else float("inf")


def scaled_cov_pp(got, ref: Reference) -> float:
    got = np.asarray(got)
    assert got.shape == ref.cov_pp.shape
    dev = np.abs(got - ref.cov_pp) / (ref.ysd**2 * np.sqrt(ref.kpp[:, None] * ref.kpp[None, :]))
    return float(dev.max()) if np.isfinite(got).all() else float("inf")


def scaled_var(got, ref: Reference, want=None) -> float:
    want = ref.var if want is None else want
    got = np.asarray(got)
    assert got.shape == want.shape
    return float((np.abs(got - want) / (ref.ysd**2 * ref.kxx)).max()) if np.isfinite(got).all() else float("inf")


def scaled_mean(got, ref: Reference, want=None) -> float:
    want = ref.mean if want is None else want
    got = np.asarray(got)
    assert got.shape == want.shape
    return float((np.abs(got - want) / ref.ysd).max()) if np.isfinite(got).all() else float("inf")


# ---- the long-double restatement (CPU guard only) -----------------------------------------------------------------------------------
def _ld_base(kind, A, B, ls, dims, alpha, period):
    """One base kernel on long-double rows A [a, c], B [b, c] (the columns it acts on), gpytorch's definitions."""
    ls = np.asarray(ls, dtype=LD)
    if kind == "linear":  # ``ls``: the variances
        return (A * ls) @ B.T
    if kind.startswith("poly"):
        return (A @ B.T + LD(alpha)) ** int(kind[-1])
    diff = A[:, None, :] - B[None, :, :]
    if kind == "periodic":
        pi = LD(4) * np.arctan(LD(1))
        return np.exp(-2 * (np.sin(pi * diff / np.asarray(period, dtype=LD)) ** 2 / ls).sum(axis=2))
    r2 = ((diff / ls) ** 2).sum(axis=2)
    if kind == "rbf":
        return np.exp(-r2 / 2)
    if kind == "rq":
        return (1 + r2 / (2 * LD(alpha))) ** (-LD(alpha))
    r = np.sqrt(r2)
    if kind == "matern52":
        s5 = np.sqrt(LD(5))
        return (1 + s5 * r + LD(5) / 3 * r2) * np.exp(-s5 * r)
    if kind == "matern32":
        s3 = np.sqrt(LD(3))
        return (1 + s3 * r) * np.exp(-s3 * r)
    if kind == "matern12":
        return np.exp(-r)
    if kind == "piecewise2":  # (1 - r)_+^(j + 2) (1 + (j + 2) r + (j^2 + 4 j + 3) / 3 r^2), j = floor(D / 2) + 3
        j = dims // 2 + 3
        return np.maximum(0, 1 - r) ** (j + 2) * (1 + (j + 2) * r + LD(j * j + 4 * j + 3) / 3 * r2)
    raise ValueError(kind)


def ld_kernel(ospec, op, A_raw, B_raw):
    """K(A, B) of the oracle's model description in long double, from raw rows: normalisation, members, outputscale, task factor."""
    lo, hi = np.asarray(ospec.lo, dtype=LD), np.asarray(ospec.hi, dtype=LD)
    A = (np.asarray(A_raw, dtype=LD)[:, ospec.num_idx] - lo) / (hi - lo)
    B = (np.asarray(B_raw, dtype=LD)[:, ospec.num_idx] - lo) / (hi - lo)
    if ospec.kernel == "rff" and not ospec.members:
        W = np.asarray(ospec.frequencies, dtype=LD) / np.asarray(op.lengthscale, dtype=LD).reshape(-1, 1)
        PA, PB = A @ W, B @ W
        K = (np.cos(PA) @ np.cos(PB).T + np.sin(PA) @ np.sin(PB).T) / W.shape[1]
    elif not ospec.members:
        c = ospec.dims_of(None)
        K = _ld_base(ospec.kernel, A[:, c], B[:, c], op.lengthscale, len(c), None if op.rq_alpha is None else op.rq_alpha[0],
                     None if op.period is None else op.period[0])
    else:
        grams = []
        for m, t in enumerate(ospec.members):
            c = ospec.dims_of(m)
            grams.append(LD(op.member_scale[m]) * _ld_base(t.kernel, A[:, c], B[:, c], op.member_ls[m], len(c),
                                                           None if op.rq_alpha is None else op.rq_alpha[m],
                                                           None if op.period is None else op.period[m]))
        if ospec.composition == "product":
            K = functools.reduce(lambda a, b: a * b, grams)
        elif ospec.composition == "sum":
            K = functools.reduce(lambda a, b: a + b, grams)
        else:
            terms: dict = {}
            for m, G in enumerate(grams):
                g = ospec.member_terms[m]
                terms[g] = G if g not in terms else terms[g] * G
            K = functools.reduce(lambda a, b: a + b, terms.values())
    if ospec.use_outputscale:
        K = K * LD(op.outputscale)
    if ospec.task_idx is not None:
        W, v = np.asarray(op.task_W, dtype=LD), np.asarray(op.task_v, dtype=LD)
        Bt = W @ W.T + np.diag(v)
        if op.target_scaled:
            Bt = Bt / Bt[0, 0]
        ta, tb = np.asarray(A_raw)[:, ospec.task_idx].astype(np.int64), np.asarray(B_raw)[:, ospec.task_idx].astype(np.int64)
        K = K * Bt[np.ix_(ta, tb)]
    return K


def ld_cholesky(A):
    """Column Cholesky in long double."""
    n = len(A)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert c[0] > 0
        L[j:, j] = c / np.sqrt(c[0])
    return L


def ld_forward(L, B):
    """L^-1 B by forward substitution in long double."""
    X = np.array(B, dtype=LD)
    for i in range(len(L)):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


@functools.lru_cache(maxsize=4)
def _ld_factor(model: PendModel):
    md = model.build()
    om = md.om
    Ky = ld_kernel(om.spec, om.params, md.Xt, md.Xt)
    Ky[np.diag_indices_from(Ky)] += np.asarray(om.params.noise_of(md.tt), dtype=LD)
    L = ld_cholesky(Ky)
    ystd = (np.asarray(md.y, dtype=LD) - np.asarray(md.y, dtype=LD).mean())
    sd = np.sqrt((ystd**2).sum() / (len(ystd) - 1)) if len(ystd) > 1 else LD(1)
    sd = sd if sd >= 1e-8 else LD(1)
    w = ld_forward(L, (ystd / sd - np.asarray(om.params.mean_of(md.tt), dtype=LD))[:, None])[:, 0]
    return L, w, sd, np.asarray(md.y, dtype=LD).mean()


def longdouble_reference(case: PendCase, rows=None):
    """(mean, var, cross) of the candidate rows ``rows`` (all by default) in long double: the formulas of ``reference`` restated."""
    md, d = case.model.build(), case.build()
    om = md.om
    L, w, sd, ybar = _ld_factor(case.model)
    cand = d.cand if rows is None else d.cand[rows]
    Vc = ld_forward(L, ld_kernel(om.spec, om.params, md.Xt, cand))
    kxx = np.array([ld_kernel(om.spec, om.params, cand[i:i + 1], cand[i:i + 1])[0, 0] for i in range(len(cand))], dtype=LD)
    mc = np.asarray(om.params.mean_of(d.tc if rows is None else d.tc[rows]), dtype=LD)
    mean = ybar + sd * (mc + Vc.T @ w)
    var = sd**2 * (kxx - (Vc * Vc).sum(axis=0))
    if case.p:
        Vp = ld_forward(L, ld_kernel(om.spec, om.params, md.Xt, d.P))
        cross = sd**2 * (ld_kernel(om.spec, om.params, cand, d.P) - Vc.T @ Vp)
    else:
        cross = np.empty((len(cand), 0), dtype=LD)
    return mean, var, cross


# ---- the case tables ----------------------------------------------------------------------------------------------------------------
A_RAGGED = (1, 15, 17, 65, 300)
A_OTHER = (16, 64, 300, 17, 65, 1, 15)


def family_a():
    out = []
    idx = 0
    for kd, d in KD_DIMS.items():
        for col, kernel in enumerate(("matern52", "matern52+tbl", "rbf", "matern32")):
            tbl = kernel.endswith("+tbl")
            icm = tbl and d in (9, 20)
            kw = dict(tasks=4) if icm else (dict(scale=True) if tbl else {})
            name = kernel.split("+")[0]
            n1 = A_RAGGED[idx % 5]
            n2 = next(n for n in A_OTHER[idx % 7:] + A_OTHER if n != n1)
            p2 = 8 if icm else (1, 2, 8)[idx % 3]
            out.append(PendCase("A", PendModel(name, d, n1, **kw), 15))
            out.append(PendCase("A", PendModel(name, d, n2, **kw), p2))
            idx += 1
    out += [PendCase("A", PendModel("matern52", 20, 513), 15), PendCase("A", PendModel("matern52", 20, 513), 2)]
    # the plain form: kd = 18, Matérn-1/2, RBF / Matérn-3/2 with a table
    out += [PendCase("A", PendModel("matern52", 70, 17), 15), PendCase("A", PendModel("matern52", 70, 64), 2),
            PendCase("A", PendModel("matern52", 70, 15, scale=True), 15),
            PendCase("A", PendModel("matern12", 9, 15), 15), PendCase("A", PendModel("matern12", 9, 65), 1),
            PendCase("A", PendModel("rbf", 9, 17, tasks=4), 15), PendCase("A", PendModel("matern32", 3, 65, scale=True), 8)]
    # ... and the same kernels at small d on a handle created under BBH_PIPELINE=0
    out += [PendCase("A", PendModel("matern52", 3, 17), 15, handle="nopipe"),
            PendCase("A", PendModel("matern52", 9, 15, tasks=4), 15, handle="nopipe"),
            PendCase("A", PendModel("rbf", 20, 65), 15, handle="nopipe"), PendCase("A", PendModel("matern32", 3, 1), 15, handle="nopipe")]
    return out


B_MODELS = (PendModel("matern52", 20, 100, layout="mixed"), PendModel("matern52", 9, 100, tasks=4, layout="mixed"))
B_ROWS = (1, 15, 16, 17, 63, 64, 65, 257)


def family_b():
    return [PendCase("B", m, p, N) for m in B_MODELS for p in (15, 2) for N in B_ROWS]


C_SWEEP_N = (20, 100, 257, 330, 400, 512, 513, 1030)
C_WIDTHS = {20: (4,), 100: (8,), 257: (16, 4), 330: (16, 8), 400: (16, 12), 512: (16, 16), 513: (16, 16, 4), 1030: (16, 16, 16, 16, 4)}


def family_c_models():
    out = [PendModel("matern52", d, n) for d in (9, 20) for n in C_SWEEP_N]
    out += [PendModel("matern52", d, 257) for d in (3, 28, 40, 62, 70)]
    out += [PendModel("rbf", 9, 330), PendModel("matern32", 9, 330), PendModel("matern52", 9, 513, tasks=4)]
    return out


def family_c():
    """Per model: (p, N) = (1, 1), (15, 49), (1, 130), (15, 130); the handles are chosen by the GPU test (n >= 257: also without a
    kernel-value cache and with global slabs)."""
    return [PendCase("C", m, p, N) for m in family_c_models() for p, N in ((1, 1), (15, 49), (1, 130), (15, 130))]


# (kernel, d, tasks): one model per (F, KD) of ``bbh_coopg_cross_launch`` - kd = ceil(max(d + 2, 2 d + 1 if periodic) / 4) rounded up to
# 2 / 4 / 6 / 8 - and every kernel kind of the generic production
D_COOPG = (("rq", 5, 0), ("piecewise2", 9, 0), ("linear", 20, 0), ("poly2", 5, 0), ("periodic", 3, 0), ("periodic", 5, 0),
           ("rq", 28, 0), ("poly2", 9, 0),
           ("product", 5, 0), ("product", 9, 3), ("scaled_sum", 20, 0), ("product", 28, 0),
           ("three", 5, 0), ("sum3", 9, 0), ("three", 20, 0), ("sum3", 28, 0),
           ("nested4", 5, 0), ("product4", 9, 0), ("nested4", 20, 0), ("nested4", 28, 0))
D_COOPG_FKD = {"rq": 1, "piecewise2": 1, "linear": 1, "poly2": 1, "periodic": 1, "product": 2, "scaled_sum": 2, "three": 3, "sum3": 3,
               "nested4": 4, "product4": 4, "matern_x_poly2": 2, "linear_plus_rbf": 2, "nested_dot": 4, "rq_first3": 3, "rq_second": 2}
# materialised K* only: a Matérn-1/2 factor, d = 31 (kd 9 has no instantiation), n = 513 (beyond the cooperative forms)
D_MATERIALISED = (PendModel("product_m12", 5, 60), PendModel("product", 31, 60), PendModel("product", 5, 513))
D_RFF = (PendModel("rff16", 5, 60), PendModel("rff64", 5, 60))


@functools.lru_cache(maxsize=None)
def factor_kinds(kernel: str):
    """The factor kinds of a generic model's built spec (they do not depend on d)."""
    return tuple(_make_spec(PendModel(kernel, 2, 1), np.zeros(2), np.ones(2)).factor_kinds)


def coopg_kd(model: PendModel):
    """``bbh_coopg_kd``: d + 2 features, 2 d + 1 once ANY factor is periodic; rounded up to an instantiated count, 0: none fits."""
    feats = max(model.d + 2, 2 * model.d + 1 if "periodic" in factor_kinds(model.kernel) else 0)
    kd = (feats + 3) // 4
    for c in (2, 4, 6, 8):
        if kd <= c:
            return c
    return 0


def family_d():
    out = []
    for kernel, d, T in D_COOPG:
        m = PendModel(kernel, d, 60, tasks=T)
        out += [PendCase("D", m, 15, 257), PendCase("D", m, 15, 65), PendCase("D", m, 15, 257, handle="nocoopgcross"),
                PendCase("D", m, 15, 65, handle="nocoopgcross")]
    out += [PendCase("D", m, 15, N) for m in D_MATERIALISED for N in (257, 65)]
    out += [PendCase("D", m, 15, 257) for m in D_RFF]
    return out


E_MODELS = (PendModel("matern52", 9, 20), PendModel("matern52", 9, 100), PendModel("matern52", 9, 100, tasks=4),
            PendModel("rff16", 5, 60), PendModel("product", 5, 60))
E_STEPS = ((15, 1), (2, 2), (0, 3), (1, 4))  # (p, pend_seed): different points each time


def expected_p0_form(model: PendModel, N: int) -> str:
    """The form ``bbh_launch_fused`` gives a variance pass WITHOUT pending columns on a default handle (``posterior_kernel_form()``):
    feature space for RFF; for the generic family the cooperative form with the generic production where it is instantiated
    (no Matérn-1/2 factor, kd <= 8, n <= 512), else the materialised K*; otherwise register-resident (n <= 128, kd <= 8, from the
    measured row count on), cooperative (n <= 512), two-sweep cooperative (n <= 1024, Matérn-5/2), windowed."""
    if model.rff:
        return "feature-space"
    if model.generic:
        return "cooperative-generic" if (model.kernel != "product_m12" and coopg_kd(model) and model.nb <= 32) else "materialised"
    kd, kernel, tbl = model.kd, model.kernel, model.has_tbl
    if kd > 16 or kernel == "matern12" or (kernel == "matern32" and tbl):
        return "windowed"
    NB = (model.n + 15) // 16
    small = model.nb <= 8 and kd <= 8 and not (NB >= 5 and (kernel == "matern32" or (kernel == "rbf" and tbl)))
    if small and N >= (0, 0, 0, 0, 0, 20000, 60000, 120000, 300000)[NB]:
        return "register-resident"
    if model.nb <= 32:
        return "cooperative"
    if model.nb <= 64 and kernel == "matern52":
        return "cooperative-2sweep"
    return "windowed"



def family_e():
    return [PendCase("E", m, p, 130, pend_seed=s) for m in E_MODELS for p, s in E_STEPS]


def all_cases():
    return family_a() + family_b() + family_c() + family_d() + family_e()


def unique_cases():
    """One case per (model, p, N, pending set): what the CPU guard checks."""
    seen, out = set(), []
    for c in all_cases():
        if c.key not in seen:
            seen.add(c.key)
            out.append(c)
    return out


# ---- deliberate defects (CPU guard): the reference restated with one thing wrong --------------------------------------------------
DEFECTS = ("shift", "stale", "task0", "padding")


def defective_cross(case: PendCase, defect: str):
    """The reference cross-covariances [N, p] with one defect, or None where the defect does not apply to the case:

      shift    columns shifted by one (p >= 2)
      stale    column p left at the point the previous pending set had there (the set of ``pend_seed + 1``; not where that is the same point)
      task0    every pending task taken as 0 (task models with a pending point outside task 0)
      padding  one padding row of the training block given a unit kernel value on both sides (the factor is the identity there)"""
    import scipy.linalg as sla

    from oracle import gp_oracle as go

    md, d, ref = case.model.build(), case.build(), case.reference()
    om, p = md.om, case.p
    if p == 0:
        return None
    if defect == "shift":
        return np.roll(ref.cross, 1, axis=1) if p >= 2 else None
    if defect == "stale":
        Uo, to = pending_points(case.model, p, case.pend_seed + 1)
        if np.array_equal(Uo[p - 1], d.Up[p - 1]):  # (n = 1: the one training row again)
            return None
        out = np.array(ref.cross)
        out[:, p - 1] = batched_cross(om, d.cand, md.assemble(case.model, Uo[p - 1:], to[p - 1:]))[:, 0]
        return out
    if defect == "task0":
        if not case.model.tasks or not d.tp.any():
            return None
        return batched_cross(om, d.cand, md.assemble(case.model, d.Up, np.zeros_like(d.tp)))
    if defect == "padding":
        Xcn, Pn = go.normalize_inputs(om.spec, d.cand), go.normalize_inputs(om.spec, d.P)
        Vc = sla.solve_triangular(om.L, go.cross_cov(om.spec, om.params, Xcn, om.Xn).T, lower=True)
        Vp = sla.solve_triangular(om.L, go.cross_cov(om.spec, om.params, Pn, om.Xn).T, lower=True)
        Vc, Vp = np.vstack([Vc, np.ones((1, len(Xcn)))]), np.vstack([Vp, np.ones((1, len(Pn)))])
        return om.ysd**2 * (go.cross_cov(om.spec, om.params, Xcn, Pn) - Vc.T @ Vp)
    raise ValueError(defect)
