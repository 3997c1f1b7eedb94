"""Train covariances whose factorisation fails at a chosen row and succeeds at a chosen level of the jitter ladder, for
tests/test_factor_ladder_gpu.py and its CPU guard, tests/test_factor_cases_cpu.py: the case table, the model builder and the
references.

``bbh_factorize`` (baybe_amd/csrc/bbh_model.hip) is gpytorch's ``psd_safe_cholesky``: a plain attempt, then 1e-8, 1e-7, 1e-6 on the
diagonal.  A model with noise-free latent rows (noise mask 0, the rows behind the training rows of an extended qLogNEHVI / qNEI model)
whose attempt fails INSIDE the latent block puts ``step / ysd^2`` on the latent rows' diagonal only - BoTorch's ladder on the latent
block's Schur complement in the target's original scale.  Which branch runs is decided by the row the device reports,
``info = 64 J + j + 1`` at the first non-positive pivot.

THE CONSTRUCTION.  Distinct training rows with short lengthscales (BAYBE preset, 0.35 x ``fixed_theta(d)[0]``, mean 0.02: the second
smallest eigenvalue of the kernel matrix stays above 0.05), row ``a`` copied into row ``b > a`` with ``y[b] = y[a]``, and a NEGATIVE noise
-0.3 j_k, j_k = 1e-8 10^(k-1): the duplicate direction then has the eigenvalue noise + jitter - -0.2 j_k or lower at every earlier
level, +0.7 j_k at level k - and the factorisation fails at row b, decisively, until level k.  Exact duplicates with zero noise are not
used: their pivot is +-1e-17 and the level a matter of rounding (tests/_joint_cases.py says the same of the joint kernels).  Noise
-3e-5 exhausts the ladder.  Equal y keeps 1 / lambda out of alpha.

Masked models: the noisy rows first, ``latent`` rows with mask 0 last, ``standardization=(ybar, 0.25)`` so that ``step`` and
``step / ysd^2`` differ by 16 x.  A pair whose b is a latent row takes the noise -0.3 j_k / ysd^2 (the pivot of b is j_latent - |noise|):
the latent branch, ``jitter`` = j_k / ysd^2.  A pair with b = n_noisy - 1 fails directly in front of the first latent row (an ``info``
one too large would take the latent branch), b = n_noisy directly behind it (one too small: the whole-diagonal branch).

References: ``oracle.gp_oracle.GPModel`` for plain models; for masked models - and for a level forced on a model - ``ladder_model``,
the same class with ``k(X, X) + diag(noise mask)`` walked through the ladder by the rule above (LAPACK's potrf names the failing row),
``scipy.linalg.cholesky`` and ``cho_solve``.  Everything is compared scaled to the prior: |mean - ref| / ysd, |var - ref| / ysd^2
(k(x, x) = 1: the preset has no outputscale), held to ``TOL`` = 1e-11."""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from _pending_cases import LD, REF_NOISE, TOL, ld_cholesky, ld_forward, ld_kernel  # noqa: F401  (TOL, REF_NOISE: re-exported)
from _problems import fixed_theta, make_grid, oracle_params, oracle_spec

JITTERS = (0.0, 1e-8, 1e-7, 1e-6)  # the ladder, as ``bbh_factorize`` and ``oracle.gp_oracle.GPModel`` walk it (1e-8 * 10**attempt)
EXHAUSTED = 4                      # k of a case no level rescues
NOISE_EXHAUSTED = -3e-5
YSD_GIVEN = 0.25                   # masked models: ysd^2 = 1 / 16
DIMS = {64: 3, 66: 3, 70: 3, 200: 5, 1030: 6}
MEAN = 0.02
N_GRID, N_TRAIN_ROWS = 200, 20     # candidates: both copies' row, 20 training rows, 200 grid rows


def level_value(k: int, unit_ysd: float | None = None) -> float:
    """j_k as the ladder computes it (``1e-8 * 10**attempt``), over ysd^2 for the latent branch."""
    if k == 0:
        return 0.0
    step = 1e-8 * 10 ** (k - 1)
    return step if unit_ysd is None else step / (unit_ysd * unit_ysd)


@dataclass(frozen=True)
class FactorModel:
    n: int
    pairs: tuple = ()   # ((a, b), ...) row a copied into row b > a; the pair with the smallest b fails first
    latent: int = 0     # trailing rows with noise mask 0

    @property
    def d(self):
        return DIMS[self.n]

    @property
    def n_noisy(self):
        return self.n - self.latent

    @property
    def masked(self):
        return self.latent > 0

    @property
    def first(self):
        """The pair whose b comes first: its pivot is the first to fail."""
        return min(self.pairs, key=lambda ab: ab[1])

    @property
    def latent_branch(self):
        return self.masked and bool(self.pairs) and self.first[1] >= self.n_noisy

    @property
    def unit_ysd(self):
        """ysd where the case's noise and level are in units of 1 / ysd^2 (the latent branch), else None."""
        return YSD_GIVEN if self.latent_branch else None

    @property
    def id(self):
        tag = "+".join(f"a{a}b{b}" for a, b in self.pairs) or "sound"
        return f"n{self.n}-{tag}" + (f"-lat{self.latent}" if self.latent else "")

    def build(self):
        return _build_model(self)


@dataclass(frozen=True)
class FactorCase:
    model: FactorModel
    k: int  # 0: well conditioned, stays at jitter 0; 1 .. 3: takes exactly that level; EXHAUSTED: the ladder runs out

    @property
    def id(self):
        return f"{self.model.id}-{'exhausted' if self.k == EXHAUSTED else f'k{self.k}'}"

    @property
    def noise(self):
        m = self.model
        if self.k == 0:
            return fixed_theta(m.d)[1]
        unit = 1.0 if m.unit_ysd is None else 1.0 / (m.unit_ysd * m.unit_ysd)
        return NOISE_EXHAUSTED * unit if self.k == EXHAUSTED else -0.3 * level_value(self.k) * unit

    @property
    def level(self):
        """What ``HipGP.jitter`` must report, exactly; None: ``ModelFittingError``."""
        return None if self.k == EXHAUSTED else level_value(self.k, self.model.unit_ysd)

    def params(self):
        from baybe_amd import gp_spec

        m = self.model
        return gp_spec.GPParams(np.full(m.d, 0.35 * fixed_theta(m.d)[0]), self.noise, MEAN)

    def reference(self):
        return _reference(self)


@dataclass(frozen=True, eq=False)
class ModelData:
    spec: object
    Xt: np.ndarray
    y: np.ndarray
    mask: np.ndarray | None        # uint8 [n] (masked models)
    standardization: tuple | None  # (ybar, ysd) handed to ``set_model`` (masked models)
    cand: np.ndarray               # [N, d]
    joint: np.ndarray              # [3, d]: a duplicated row, a grid row, another training row


@functools.lru_cache(maxsize=None)
def _build_model(fm: FactorModel) -> ModelData:
    from baybe_amd import gp_spec

    n, d = fm.n, fm.d
    seed = 100 * n + d
    G = np.unique(make_grid(4 * n + 500, d, seed), axis=0)  # distinct rows (sorted) ...
    rng = np.random.default_rng(seed + 1)
    G = G[rng.permutation(len(G))]                            # ... in no order ...
    assert len(G) >= n
    Xt = G[:n].copy()
    y = -((Xt - 0.5) ** 2).sum(1) + 0.1 * np.sin(2 * np.pi * Xt[:, 0]) + 0.05 * rng.standard_normal(n)
    for a, b in fm.pairs:                                     # ... then the planted pairs
        assert 0 <= a < b < n
        Xt[b], y[b] = Xt[a], y[a]
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    mask = std = None
    if fm.masked:
        mask = np.concatenate([np.ones(fm.n_noisy, np.uint8), np.zeros(fm.latent, np.uint8)])
        std = (float(y[: fm.n_noisy].mean()), YSD_GIVEN)
    a, b = fm.first if fm.pairs else (0, n - 1)
    others = [i for i in rng.permutation(n) if i not in (a, b)][:N_TRAIN_ROWS]
    grid = make_grid(N_GRID, d, seed + 2)
    cand = np.vstack([Xt[[a, b]], Xt[others], grid])
    joint = np.vstack([Xt[b], grid[0], Xt[others[0]]])
    out = ModelData(spec, Xt, y, mask, std, cand, joint)
    for arr in (Xt, y, cand, joint) + (() if mask is None else (mask,)):
        arr.setflags(write=False)
    return out


# ---- the references -----------------------------------------------------------------------------------------------------------------
def potrf_info(A: np.ndarray):
    """(lower factor, 0) or (None, failing row, 1-based) of LAPACK's potrf."""
    import scipy.linalg as sla

    c, info = sla.lapack.dpotrf(A, lower=1)
    return (np.tril(c), 0) if info == 0 else (None, int(info))


def walk_ladder(K: np.ndarray, mask: np.ndarray, ysd: float):
    """The ladder of ``bbh_factorize`` on K = k(X, X) + diag(noise mask).  Returns (diag, level, infos): what the successful attempt
    added to the diagonal [n] and the level it reports - (None, None, infos) when the fourth attempt fails as well -, and the failing
    row (1-based) of every failed attempt."""
    jit = jit_latent = 0.0
    infos = []
    for attempt in range(4):
        diag = np.where(mask != 0, jit, jit_latent)
        _, info = potrf_info(K + np.diag(diag))
        if info == 0:
            return diag, (jit if jit > 0.0 else jit_latent), tuple(infos)
        infos.append(info)
        step = 1e-8 * 10**attempt
        if mask[info - 1] == 0 and jit == 0.0:
            jit_latent = step / (ysd * ysd)
        else:
            jit = jit_latent = step
    return None, None, tuple(infos)


@functools.lru_cache(maxsize=None)
def _ladder_class():
    import scipy.linalg as sla
    from dataclasses import dataclass as dc

    from oracle import gp_oracle as go

    @dc
    class LadderModel(go.GPModel):
        """``GPModel`` with a noise mask, a given standardisation and the two-branch ladder (or a forced diagonal)."""

        mask: np.ndarray = None
        standardization: tuple = None
        forced: np.ndarray = None  # [n] added to the diagonal instead of walking the ladder
        infos: tuple = ()

        def __post_init__(self):
            self.X_train = np.ascontiguousarray(self.X_train, dtype=np.float64)
            self.Xn = go.normalize_inputs(self.spec, self.X_train)
            if self.standardization is None:
                self.ystd, self.ybar, self.ysd = go.standardize_targets(self.y_train)
            else:
                self.ybar, self.ysd = self.standardization
                self.ystd = (np.asarray(self.y_train, dtype=np.float64) - self.ybar) / self.ysd
            mask = np.ones(len(self.Xn)) if self.mask is None else np.asarray(self.mask, dtype=np.float64)
            K = go.cross_cov(self.spec, self.params, self.Xn, self.Xn) + np.diag(self.params.noise * mask)
            if self.forced is None:
                diag, level, self.infos = walk_ladder(K, mask, self.ysd)
                if diag is None:
                    raise sla.LinAlgError("train covariance not PD even with jitter")
                self.jitter = level
            else:
                diag = self.forced
            self.diag = diag
            self.L = sla.cholesky(K + np.diag(diag), lower=True)
            self.alpha = sla.cho_solve((self.L, True), self.ystd - self.params.mean)

    return LadderModel


def ladder_model(case: FactorCase, forced=None):
    """The numpy / scipy restatement at the case's parameters: the ladder by the device's rule, or ``forced`` [n] on the diagonal."""
    md = case.model.build()
    return _ladder_class()(oracle_spec(md.spec), oracle_params(md.spec, case.params()), md.Xt, md.y, mask=md.mask,
                           standardization=md.standardization, forced=forced)


def oracle_model(case: FactorCase):
    """The model the device is held to: ``GPModel`` for plain models (raises ``LinAlgError`` where the ladder runs out), the
    restatement for masked ones."""
    from oracle import gp_oracle as go

    md = case.model.build()
    if case.model.masked:
        return ladder_model(case)
    return go.GPModel(oracle_spec(md.spec), oracle_params(md.spec, case.params()), md.Xt, md.y)


@dataclass(frozen=True, eq=False)
class Reference:
    level: float | None   # None: the ladder is exhausted (no other field is set then)
    ysd: float = 1.0
    mean: np.ndarray = None    # [N]
    var: np.ndarray = None     # [N]
    jmean: np.ndarray = None   # [3]
    jcov: np.ndarray = None    # [3, 3]
    train: np.ndarray = None   # [n] posterior mean of the training rows


def quantities(om, md: ModelData) -> Reference:
    """Everything the device is compared on, from a ``GPModel``-like object."""
    mean, var = om.posterior(md.cand)
    jmean, jcov = om.posterior_joint(md.joint)
    out = Reference(float(om.jitter), float(om.ysd), mean, var, jmean, jcov, om.posterior(md.Xt)[0])
    for a in (out.mean, out.var, out.jmean, out.jcov, out.train):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(case: FactorCase) -> Reference:
    """Computed once per case and shared (read-only)."""
    import scipy.linalg as sla

    try:
        om = oracle_model(case)
    except sla.LinAlgError:
        return Reference(None)
    return quantities(om, case.model.build())


def deviations(ref: Reference, mean=None, var=None, jmean=None, jcov=None, train=None) -> dict:
    """Scaled deviations (the largest over the rows, every row held) of whatever is given; inf where a value is not finite."""
    out = {}
    for name, got, want, scale in (("mean", mean, ref.mean, ref.ysd), ("var", var, ref.var, ref.ysd**2), ("jmean", jmean, ref.jmean, ref.ysd),
                                   ("jcov", jcov, ref.jcov, ref.ysd**2), ("train", train, ref.train, ref.ysd)):
        if got is None:
            continue
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        out[name] = float((np.abs(got - want) / scale).max()) if np.isfinite(got).all() else float("inf")
    return out


# ---- CPU-side restatements (tests/test_factor_cases_cpu.py) ---------------------------------------------------------------------------
def deciding_pivot(A: np.ndarray):
    """Column Cholesky of A up to its first non-positive pivot: (row, pivot) of that pivot (1-based row), or (0, smallest pivot)."""
    n = len(A)
    L = np.zeros((n, n))
    smallest = np.inf
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0.0:
            return j + 1, float(c[0])
        smallest = min(smallest, float(c[0]))
        L[j:, j] = c / np.sqrt(c[0])
    return 0, smallest


def schur_ladder(K: np.ndarray, mask: np.ndarray, ysd: float):
    """BoTorch's order for a masked model: the noisy block through the plain ladder, then the latent block's Schur complement, in the
    target's original scale (x ysd^2), through the ladder again.  Returns (level of the noisy block, level of the Schur complement)."""
    import scipy.linalg as sla

    nz = np.nonzero(mask != 0)[0]
    lt = np.nonzero(mask == 0)[0]

    def plain(A):
        for j in JITTERS:
            L, info = potrf_info(A + j * np.eye(len(A)))
            if info == 0:
                return j, L
        return None, None

    j1, L = plain(K[np.ix_(nz, nz)])
    if j1 is None:
        return None, None
    V = sla.solve_triangular(L, K[np.ix_(nz, lt)], lower=True)
    S = ysd**2 * (K[np.ix_(lt, lt)] - V.T @ V)
    return j1, plain(0.5 * (S + S.T))[0]


@functools.lru_cache(maxsize=2)
def _ld_kernels(fm: FactorModel):
    from baybe_amd import gp_spec

    md = fm.build()
    ospec = oracle_spec(md.spec)
    op = oracle_params(md.spec, gp_spec.GPParams(np.full(fm.d, 0.35 * fixed_theta(fm.d)[0]), 0.0, MEAN))
    rows = np.vstack([md.cand, md.joint])
    return ld_kernel(ospec, op, md.Xt, md.Xt), ld_kernel(ospec, op, md.Xt, rows), ld_kernel(ospec, op, md.joint, md.joint)


def longdouble_reference(case: FactorCase, diag: np.ndarray):
    """(mean [N], var [N], jmean [3], jcov [3, 3]) in long double with ``diag`` on top of the noise: the reference's formulas restated
    (column Cholesky, forward substitution; the training rows among the candidates stand for ``train``)."""
    md = case.model.build()
    Kxx, Kxc, Kjj = _ld_kernels(case.model)
    mask = np.ones(case.model.n) if md.mask is None else md.mask
    Ky = Kxx.copy()
    Ky[np.diag_indices_from(Ky)] += LD(case.noise) * np.asarray(mask, dtype=LD) + np.asarray(diag, dtype=LD)
    L = ld_cholesky(Ky)
    y = np.asarray(md.y, dtype=LD)
    if md.standardization is None:
        ybar = y.mean()
        sd = np.sqrt(((y - ybar) ** 2).sum() / (len(y) - 1))
    else:
        ybar, sd = LD(md.standardization[0]), LD(md.standardization[1])
    w = ld_forward(L, ((y - ybar) / sd - LD(MEAN))[:, None])[:, 0]
    V = ld_forward(L, Kxc)
    mean = ybar + sd * (LD(MEAN) + V.T @ w)
    N = len(md.cand)
    var = sd**2 * (1 - (V[:, :N] * V[:, :N]).sum(axis=0))
    return mean[:N], var, mean[N:], sd**2 * (Kjj - V[:, N:].T @ V[:, N:])


# ---- the case tables --------------------------------------------------------------------------------------------------------------------
# positions of b (the failing row is b + 1): the second row; around the 16-row sub-block edge and the 64-row block edge; the last row with
# no padding behind it (n = 64), with padding (70, 200), in the last block row of a 17-block matrix (1030: np = 1088)
PLAIN_MODELS = (
    FactorModel(64, ((0, 1),)), FactorModel(64, ((3, 15),)), FactorModel(64, ((3, 16),)), FactorModel(64, ((3, 17),)),
    FactorModel(64, ((5, 63),)),
    FactorModel(70, ((0, 1),)), FactorModel(70, ((3, 16),)), FactorModel(70, ((5, 63),)), FactorModel(70, ((5, 64),)),
    FactorModel(70, ((5, 65),)), FactorModel(70, ((5, 69),)),
    FactorModel(200, ((3, 15),)), FactorModel(200, ((3, 17),)), FactorModel(200, ((63, 64),)), FactorModel(200, ((5, 127),)),
    FactorModel(200, ((5, 128),)), FactorModel(200, ((5, 199),)),
    FactorModel(200, ((5, 70), (100, 150))),  # two pairs in different blocks: the first one decides
    FactorModel(1030, ((5, 1023),)), FactorModel(1030, ((5, 1024),)), FactorModel(1030, ((0, 1029),)),
)
SOUND_MODELS = tuple(FactorModel(n) for n in (64, 70, 200, 1030))
# n = 66 with 12 latent rows (54 noisy), n = 200 with 72 (first latent row 128, a block edge).  Inside the latent block; directly in
# front of the first latent row (whole-diagonal ladder) and directly behind it (latent); a noisy pair in front of a latent pair (the
# first one decides: whole diagonal)
MASKED_MODELS = (
    FactorModel(66, ((5, 60),), latent=12), FactorModel(66, ((5, 53),), latent=12), FactorModel(66, ((5, 54),), latent=12),
    FactorModel(200, ((5, 150),), latent=72), FactorModel(200, ((5, 127),), latent=72), FactorModel(200, ((5, 128),), latent=72),
    FactorModel(200, ((5, 70), (100, 150)), latent=72),
)
SOUND_MASKED = (FactorModel(66, latent=12), FactorModel(200, latent=72))


def ladder_cases():
    out = [FactorCase(m, k) for m in PLAIN_MODELS + MASKED_MODELS for k in (1, 2, 3, EXHAUSTED)]
    return out + [FactorCase(m, 0) for m in SOUND_MODELS + SOUND_MASKED]


# the fit evaluation: every plain position of b under every form reachable at its size (variants of tests/_fit_cases.py::VARIANTS;
# "reg": BBH_POTRF_TILES=0 BBH_POTRF_REG=1, the per-step launches with the one-wave register kernel)
FIT_VARIANTS = {64: ("small1", "small0"), 70: ("0", "1", "2", "3", "1-gram0", "1-steps", "reg"),
                200: ("0", "1", "2", "3", "1-gram0", "1-steps", "reg"), 1030: ("0", "1")}
FIT_NOISE_FAILS, FIT_NOISE_HOLDS = -0.3e-8, 0.7e-8


def fit_expected_form(n: int, variant: str) -> set:
    """Forms ``fit_evaluation_form`` may report for the BAYBE preset at n rows under ``variant`` (``FitCase.expected_forms``)."""
    from _fit_cases import FitCase

    md = FactorModel(n).build()
    if variant == "reg":
        return {"steps+tail"}
    return FitCase("baybe", n, d=DIMS[n]).expected_forms(md.spec, variant)


def fit_point(fm: FactorModel):
    """A sound parameter point for the evaluation behind a failed one: the preset's initial values, perturbed as the fit tests do."""
    from baybe_amd import gp_spec

    md = fm.build()
    p = gp_spec.initial_params(md.spec)
    p.lengthscale = p.lengthscale * (0.7 + 0.6 * np.random.default_rng(fm.n).random(md.spec.dn))
    p.mean = 0.1
    return p
