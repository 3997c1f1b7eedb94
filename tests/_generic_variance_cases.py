"""Models, candidates and oracle references for tests/test_generic_variance_gpu.py (and its CPU guard,
tests/test_generic_variance_cases_cpu.py): the variance pass of the cooperative form with the generic production,
``bbh_coopg_posterior_kernel<KD, F>`` (csrc/bbh_coopg.h) - Product / Additive kernels of up to four factors, RQ, piecewise polynomial,
Linear, Polynomial and Periodic, n <= 512 - and, where they share ``coopg_produce``, the cross pass ``bbh_coopg_cross_kernel``.

Everything is built on tests/_pending_cases.py: a case is a ``PendCase`` with p = 0 (family V5 also p = 2), its candidates come from
``_build_case`` (rows 0 ... 4 are ``train:0``, ``train:n/2``, ``train:n-1`` and the two corners, N = 257 ends on ``train:n-1`` and a
corner), the reference is the oracle (``reference_of``), the deviations are ``scaled_mean`` / ``scaled_var`` / ``scaled_cross`` held to
``TOL`` = 1e-11, and the CPU guard holds the float64 oracle to ``REF_NOISE`` = 1e-13 of ``longdouble_reference`` - mean and variance.

What the kernel reads off a model (``bbh_launch_fused`` / ``bbh_pack_operands``): F factors; KD = ceil(feats / 4) rounded up to 2 / 4 /
6 / 8 with feats = d + 2, or 2 d + 1 once a factor is periodic; nb = 4 ceil(n / 64) column blocks of 16 and the first round
g0 = 8 - nb / 4 (the model occupies the LAST rounds); one workgroup per 16 candidates.

  V1  every instantiation (F 1 ... 4 x KD 2, 4, 6, 8), every kind of the generic production, one model under the ICM table, ragged n
      (never a multiple of 16) such that each g0 in 0 ... 7 occurs at least twice; N = 257: sixteen full tiles and a lone row
  V2  the rounds: a two-factor model with a table in the mixed layout and the widest instantiation (KD 8, F 4) at
      n = 1 ... 512, and n = 513 of each, which is the materialised K*
  V3  ragged tiles and layout: N = 1 ... 257 rows of a strided view into buffers with sentinels behind row N (the GPU test)
  V4  feature slots: Product at d = 6, 14, 22, 30 fills every slot of KD 2, 4, 6, 8 (d + 2 = 4 KD) and d = 7, 15, 23 starts the next
      count; Periodic at d = 3 | 4, 7 | 8, 11 | 12, 15 ends and starts a count (2 d + 1 = 31 at d = 15: the last slot but one);
      Product d 31 and Periodic d 16 have no instantiation
  V5  far rows under a heavy tail: RQ with alpha = 0.4 and lengthscales 1e-4 U[0.8, 1.2], where r^2 > 1e7 for nearly every
      (candidate, training) pair and k = (1 + r^2 / 2 alpha)^-alpha is still 1e-3 there - a production that takes a large metric for
      the mark of a padding row returns the prior.  The candidates are ORDINARY rows only and the pending points grid rows: at these
      lengthscales |a|^2 + |b|^2 - 2 a.b has an absolute error near 1e-7, which a coincident row's r^2 = 0 cannot survive - a
      property of the expanded distance, not what this family is after; the smallest non-zero r^2 is near 7e5, a relative error of
      1e-13.  ``rq`` alone and ``rq_first3`` / ``rq_second`` with every factor at those lengthscales (in the two products the Matérn
      factor is 0 at such a distance: the posterior is the prior whatever the production does - the controls), and the two products
      with the RQ factor alone at those lengthscales: RQ first, where factor 0 carries the large metric, and RQ second, where it
      does not
  V6  handle state: five loads on one handle (``V6_STEPS``), each held to the oracle and to a fresh handle's bits

Noise: at ``fixed_theta``'s e^-5 the float64 oracle's mean is not within 1e-13 of its long-double restatement for the low-rank kinds at
large n (Linear d 20 n 512: 2.6e-12; Polynomial(2) d 9: 2.0e-12; piecewise d 9: 8.6e-13); at noise 0.2 it is (7e-14).  The single
Linear, Polynomial and piecewise models of these families therefore have noise 0.2 (``model``)."""

from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass

import numpy as np

import _pending_cases as pc
from _pending_cases import CaseData, PendCase, PendModel, N_FULL
from _problems import fixed_theta

LOW_RANK = ("linear", "poly2", "piecewise2")
N_SMALL = 49
FAR_R2 = 1e7


def model(kernel, d, n, **kw):
    if kernel in LOW_RANK:
        kw.setdefault("noise", 0.2)
    return PendModel(kernel, d, n, **kw)


@dataclass(frozen=True)
class VarCase(PendCase):
    ordinary: bool = False   # V5: the ordinary rows of the candidate set only, every pending point a grid row

    @property
    def key(self):
        return self.model, self.p, self.N, self.pend_seed, self.ordinary

    def build(self):
        return _build_ordinary(self.model, self.p, self.N) if self.ordinary else pc._build_case(self.model, self.p, self.N, self.pend_seed)

    def reference(self):
        return _reference_ordinary(self.model, self.p, self.N) if self.ordinary else pc._reference(self.model, self.p, self.N, self.pend_seed)


@functools.lru_cache(maxsize=None)
def _build_ordinary(m: PendModel, p: int, N: int) -> CaseData:
    md = m.build()
    full = pc._build_case(m, 0, N_FULL, 0)
    keep = np.nonzero(full.rows("ordinary"))[0][:N]
    assert len(keep) == N and not m.tasks
    Up, tp = md.pool[N_FULL:N_FULL + p].copy(), np.zeros(p, dtype=np.int64)
    out = CaseData(np.ascontiguousarray(full.cand[keep]), md.assemble(m, Up, tp) if p else np.empty((0, m.dtot)), ("ordinary",) * N,
                   full.Uc[keep], full.tc[keep], Up, tp)
    for a in (out.cand, out.P, out.Uc, out.tc, out.Up, out.tp):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference_ordinary(m: PendModel, p: int, N: int):
    return pc.reference_of(m, _build_ordinary(m, p, N))


def g0_of(m: PendModel) -> int:
    return 8 - m.nb // 4


def n_factors(m: PendModel) -> int:
    return pc.D_COOPG_FKD[m.kernel]


# ---- V1 ---------------------------------------------------------------------------------------------------------------------------
V1_EXTRA = (("matern_x_poly2", 9, 0), ("linear_plus_rbf", 20, 0), ("nested_dot", 5, 0), ("nested_dot", 14, 0), ("rq_first3", 28, 0))
V1_N = (60, 65, 130, 193, 257, 321, 385, 449, 511)


# Periodic d 3 at n = 257 - 257 rows of a smooth kernel on three columns - has noise 0.05: at e^-5 the float64 oracle's mean lies 2.0e-13
# from its long-double restatement (the guard's bound is 1e-13)
V1_NOISE = {("periodic", 3): 0.05}


def v1_models():
    return [model(k, d, V1_N[i % len(V1_N)], tasks=T, **({"noise": V1_NOISE[k, d]} if (k, d) in V1_NOISE else {}))
            for i, (k, d, T) in enumerate(pc.D_COOPG + V1_EXTRA)]


def family_v1():
    return [VarCase("V1", m, 0, N_FULL) for m in v1_models()]


# ---- V2 ---------------------------------------------------------------------------------------------------------------------------
V2_N = (1, 16, 17, 64, 65, 128, 129, 193, 256, 257, 321, 385, 448, 449, 511, 512)


def v2_models(n):
    return [model("product", 9, n, tasks=3, layout="mixed"), model("nested_dot", 14, n)]


def family_v2():
    return [VarCase("V2", m, 0, N_SMALL) for n in V2_N + (513,) for m in v2_models(n)]


# ---- V3 ---------------------------------------------------------------------------------------------------------------------------
V3_MODELS = (model("linear_plus_rbf", 20, 100), model("product", 9, 100, tasks=3, layout="mixed"))
V3_ROWS = (1, 15, 16, 17, 31, 33, 257)


def family_v3():
    return [VarCase("V3", m, 0, N) for m in V3_MODELS for N in V3_ROWS]


# ---- V4 ---------------------------------------------------------------------------------------------------------------------------
V4_PRODUCT_D = (6, 7, 14, 15, 22, 23, 30)
V4_PERIODIC_D = (3, 4, 7, 8, 11, 12, 15)
V4_FULL_SLOT_D = (6, 14, 22, 30)
V4_OUT_OF_RANGE = (model("product", 31, 60), model("periodic", 16, 60))


def features(m: PendModel) -> int:
    return 2 * m.d + 1 if "periodic" in pc.factor_kinds(m.kernel) else m.d + 2


def family_v4():
    ms = [model("product", d, 60) for d in V4_PRODUCT_D] + [model("periodic", d, 60) for d in V4_PERIODIC_D] + list(V4_OUT_OF_RANGE)
    return [VarCase("V4", m, 0, N_SMALL) for m in ms]


# ---- V5 ---------------------------------------------------------------------------------------------------------------------------
def _ls_factor(F, d=5, target=1e-4):
    """What the default lengthscales ls0 sqrt(F) U[0.8, 1.2] of a product of F factors are multiplied by to become target U[0.8, 1.2]."""
    return target / (fixed_theta(d)[0] * np.sqrt(F))


V5_ALL = (model("rq", 5, 60, ls_scale=_ls_factor(1), rq_alpha=0.4), model("rq_first3", 5, 60, ls_scale=_ls_factor(3), rq_alpha=0.4),
          model("rq_second", 5, 60, ls_scale=_ls_factor(2), rq_alpha=0.4))
V5_RQ_ONLY = (model("rq_first3", 5, 60, rq_ls_scale=_ls_factor(3), rq_alpha=0.4),
              model("rq_second", 5, 60, rq_ls_scale=_ls_factor(2), rq_alpha=0.4))
V5_MODELS = V5_ALL + V5_RQ_ONLY
# the models a production that zeroes every row with a factor-0 metric beyond 1e7 gets wrong; in the others the large metric is not
# factor 0's (``rq_second`` with the RQ factor alone far) or a Matérn factor is 0 there anyway
V5_SENSITIVE = (V5_ALL[0], V5_RQ_ONLY[0])
V5_P = 2


def family_v5():
    return [VarCase("V5", m, p, N_SMALL, ordinary=True) for m in V5_MODELS for p in (0, V5_P)]


def rq_factor(m: PendModel) -> int:
    return pc.factor_kinds(m.kernel).index("rq")


def factor_metric(m: PendModel, f: int, A_raw, B_raw):
    """The oracle's metric of factor f (r^2 of a distance kind) between raw rows."""
    from oracle import gp_oracle as go

    om = m.build().om
    A, B = (go.normalize_inputs(om.spec, X)[:, om.spec.num_idx] for X in (A_raw, B_raw))
    if om.spec.members:
        c, t = om.spec.dims_of(f), om.spec.members[f]
        return go._metric(t.kernel, A[:, c], B[:, c], om.params.member_ls[f], go._period_of(om.params, f))
    c = om.spec.dims_of(None)
    return go._metric(om.spec.kernel, A[:, c], B[:, c], om.params.lengthscale, go._period_of(om.params, 0))


# ---- V6 ---------------------------------------------------------------------------------------------------------------------------
# one handle: a two-factor model; a four-factor model of the same fragment volume ((nb + 1) KD 64 F doubles: KD 4 F 2 = KD 2 F 4), so that
# the per-factor buffers are kept; a single Matérn kernel, which takes the generic production away (``coopg_ready`` false); the first
# model again; a new factorisation of it with every lengthscale x 1.1 (the same data: the rows do not depend on ``ls_scale``)
V6_STEPS = (model("product", 9, 130), model("nested4", 5, 130), PendModel("matern52", 9, 130), model("product", 9, 130),
            model("product", 9, 130, ls_scale=1.1))


def family_v6():
    return [VarCase("V6", m, 0, N_SMALL) for m in V6_STEPS[:3] + V6_STEPS[4:]]


def all_cases():
    return family_v1() + family_v2() + family_v3() + family_v4() + family_v5() + family_v6()


def unique_cases():
    seen, out = set(), []
    for c in all_cases():
        if c.key not in seen:
            seen.add(c.key)
            out.append(c)
    return out


# ---- deliberate defects (CPU guard): the reference restated with one thing wrong ------------------------------------------------------
DEFECTS = ("padding", "kself", "plainsum", "swap", "lastslot", "far")


def restated(case: PendCase, Ks=None, kxx=None, KsP=None):
    """(mean, var, cross) of the case from the oracle's factorisation with K(X*, X) [N, n], k(x, x) [N] and K(P, X) [p, n] as given."""
    import scipy.linalg as sla

    from oracle import gp_oracle as go

    om, d = case.model.build().om, case.build()
    Xcn = go.normalize_inputs(om.spec, d.cand)
    Ks = go.cross_cov(om.spec, om.params, Xcn, om.Xn) if Ks is None else Ks
    kxx = go.prior_var(om.spec, om.params, Xcn) if kxx is None else kxx
    mu = om.params.mean_of(go.task_rows(om.spec, Xcn)) + Ks @ om.alpha
    V = sla.solve_triangular(om.L, Ks.T, lower=True)
    cross = np.empty((len(Xcn), 0))
    if case.p:
        Pn = go.normalize_inputs(om.spec, d.P)
        KsP = go.cross_cov(om.spec, om.params, Pn, om.Xn) if KsP is None else KsP
        cross = om.ysd**2 * (go.cross_cov(om.spec, om.params, Xcn, Pn) - V.T @ sla.solve_triangular(om.L, KsP.T, lower=True))
    return om.ybar + om.ysd * mu, om.ysd**2 * (kxx - (V * V).sum(axis=0)), cross


def prior_k0(m: PendModel):
    """``CoopGArgs::prior_k0`` times the outer outputscale: k(x, x) with every factor's k_f(x, x) taken as 1."""
    from oracle import gp_oracle as go

    om = m.build().om
    assert om.spec.task_idx is None
    k0 = float(go.compose_members(om.spec, [np.array([s]) for s in om.params.member_scale])[0]) if om.spec.members else 1.0
    return k0 * (om.params.outputscale if om.spec.use_outputscale else 1.0)


def defective(case: PendCase, defect: str):
    """(mean, var, cross) with one defect, or None where the defect does not apply to the case:

      padding   one padding row of the training blocks given a unit kernel value (n no multiple of 64)
      kself     k(x, x) taken as the constant ``prior_k0`` (models with a dot kind)
      plainsum  the grouped combine taken as a plain sum (``nested*``)
      swap      two factors' scales exchanged (sums and grouped sums with unequal scales; a product's scales commute)
      lastslot  the last feature slot - the constant that meets |b|^2 - dropped (Product at d + 2 = 4 KD)
      far       every training row whose factor-0 r^2 exceeds 1e7 zeroed (V5)"""
    from oracle import gp_oracle as go

    m = case.model
    md, d, ref = m.build(), case.build(), case.reference()
    om = md.om
    kinds = pc.factor_kinds(m.kernel) if m.generic else ()
    Xcn = go.normalize_inputs(om.spec, d.cand)
    if defect == "padding":
        if m.n % 64 == 0:
            return None
        return ref.mean, ref.var - om.ysd**2, ref.cross - om.ysd**2  # (its alpha is 0: the mean stays)
    if defect == "kself":
        if not any(k == "linear" or k.startswith("poly") for k in kinds):
            return None
        return restated(case, kxx=np.full(len(Xcn), prior_k0(m)))
    if defect == "plainsum":
        if not m.kernel.startswith("nested"):
            return None
        flat = dataclasses.replace(om.spec, composition="sum", member_terms=None)
        return restated(case, Ks=go.cross_cov(flat, om.params, Xcn, om.Xn), kxx=go.prior_var(flat, om.params, Xcn))
    if defect == "swap":
        if not om.spec.members or om.spec.composition == "product":
            return None
        sc = np.array(om.params.member_scale, dtype=float)
        pairs = [(i, j) for i in range(len(sc)) for j in range(i + 1, len(sc)) if sc[i] != sc[j]
                 and (om.spec.composition == "sum" or om.spec.member_terms[i] != om.spec.member_terms[j])]
        if not pairs:
            return None
        i, j = pairs[0]
        p2 = om.params.copy()
        p2.member_scale = sc.copy()
        p2.member_scale[[i, j]] = sc[[j, i]]
        return restated(case, Ks=go.cross_cov(om.spec, p2, Xcn, om.Xn), kxx=go.prior_var(om.spec, p2, Xcn))
    if defect == "lastslot":
        if not (case.family == "V4" and m.kernel == "product" and m.d in V4_FULL_SLOT_D):
            return None
        # train [-2 a, |a|^2, 1] . candidate [b, 1, |b|^2] without its last term, a = (xn - 1/2) / l; floored at 0 like the kernel's r^2
        A, B = Xcn[:, om.spec.num_idx] - 0.5, om.Xn[:, om.spec.num_idx] - 0.5
        grams = []
        for f, t in enumerate(om.spec.members):
            ls = np.asarray(om.params.member_ls[f])
            b2 = ((A / ls) ** 2).sum(axis=1)[:, None]
            r2 = np.maximum(factor_metric(m, f, d.cand, md.Xt) - b2, 0.0)
            grams.append(om.params.member_scale[f] * go.base_kernel_from_r2(t.kernel, r2, m.d, None))
        return restated(case, Ks=grams[0] * grams[1])
    if defect == "far":
        if case.family != "V5":
            return None
        Ks = np.where(factor_metric(m, 0, d.cand, md.Xt) > FAR_R2, 0.0, go.cross_cov(om.spec, om.params, Xcn, om.Xn))
        KsP = None
        if case.p:
            Pn = go.normalize_inputs(om.spec, d.P)
            KsP = np.where(factor_metric(m, 0, d.P, md.Xt) > FAR_R2, 0.0, go.cross_cov(om.spec, om.params, Pn, om.Xn))
        return restated(case, Ks=Ks, KsP=KsP)
    raise ValueError(defect)


def moved(case: PendCase, bad) -> float:
    """How far a defective restatement lies from the reference, in the units the device is held in."""
    ref = case.reference()
    return max(pc.scaled_mean(bad[0], ref), pc.scaled_var(bad[1], ref), pc.scaled_cross(bad[2], ref) if case.p else 0.0)
