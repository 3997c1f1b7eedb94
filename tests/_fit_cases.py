"""The case table of tests/test_fit_forms_gpu.py (and of its CPU guard, tests/test_fit_cases_cpu.py): models, sizes and switches
that steer one fit evaluation (``bbh_fit_value_grad``) down each of its device paths, the path each row is built for, and the
oracle side of the comparison.

np is n rounded up to 64.  ``bbh_fit_enqueue`` (baybe_amd/csrc/bbh_model.hip) picks the path from np, the model (one kernel
factor, no per-task likelihood, dn <= 32, T <= 4, theta length <= 49, not periodic: ``bbh_fit_flow_eligible``) and the
``BBH_*`` switches a handle reads when it is created; ``HipGP.fit_evaluation_form`` reads back which one ran."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from _problems import make_problem, oracle_params, oracle_spec

# device tolerances (value / gradient per slot against the analytic oracle; objective against the autograd oracle)
VALUE_RTOL, VALUE_ATOL = 1e-10, 1e-11
GRAD_RTOL, GRAD_ATOL_OF_MAX = 1e-8, 1e-10
OBJ_RTOL, OBJ_GRAD_RTOL, OBJ_GRAD_ATOL_OF_MAX = 1e-10, 1e-7, 1e-9

# the switches of each variant (a handle reads them when it is created)
VARIANTS = {
    "small1": {"BBH_FIT_SMALL": "1"},
    "small0": {"BBH_FIT_SMALL": "0"},
    "0": {"BBH_FIT_FLOW": "0"},
    "1": {"BBH_FIT_FLOW": "1"},
    "2": {"BBH_FIT_FLOW": "2"},
    "3": {"BBH_FIT_FLOW": "3"},
    "1-mt0": {"BBH_TILE_MT": "0"},
    "1-mtp": {"BBH_TILE_MT": "partial"},
    "1-gram0": {"BBH_TILE_GRAM": "0"},
    "1-wt0": {"BBH_TILE_WT": "0"},
    "1-copy": {"BBH_TILE_GRAM_THETA": "copy"},
    "1-steps": {"BBH_POTRF_TILES": "0"},
}
ALL_VARIANTS_UP_TO_1024 = ("0", "1", "2", "3", "1-mt0", "1-mtp", "1-gram0", "1-wt0", "1-copy", "1-steps")
FORMS = ("launch", "small", "tiles+mt", "tiles+mt-partial", "tiles", "gram+tiles", "one-launch", "split", "rff", "steps+tail")
# block rows up to which the tile-dataflow factorisation surely has room for all of K^-1's tiles beside its own (13 on 256 CUs:
# test_m_tile_edge finds the exact edge through the read-back)
MT_SURE_NBK = 8


def _space(d):
    class Space:
        comp_rep_columns = tuple(f"x{j}" for j in range(d)) + ("task",)

    return Space()


def _kernel(name):
    from baybe_amd.kernels import (GammaPrior, LinearKernel, MaternKernel, PeriodicKernel, PiecewisePolynomialKernel, PolynomialKernel,
                                   ProductKernel, RBFKernel, RQKernel, ScaleKernel)

    os_prior = GammaPrior(2, 0.5)
    return {
        "m12": ScaleKernel(MaternKernel(0.5, GammaPrior(3, 1)), os_prior),
        "m32": ScaleKernel(MaternKernel(1.5, GammaPrior(3, 1)), os_prior),
        "rbf": ScaleKernel(RBFKernel(GammaPrior(3, 1)), os_prior),
        "rq": ScaleKernel(RQKernel(GammaPrior(3, 1)), os_prior),
        "pp0": ScaleKernel(PiecewisePolynomialKernel(0, GammaPrior(3, 1)), os_prior),
        "pp2": ScaleKernel(PiecewisePolynomialKernel(2, GammaPrior(3, 1)), os_prior),
        "linear": ScaleKernel(LinearKernel(), os_prior),
        "poly": PolynomialKernel(2),
        "periodic": ScaleKernel(PeriodicKernel(GammaPrior(3, 1)), os_prior),
        "subset": ScaleKernel(MaternKernel(1.5, GammaPrior(3, 1), parameter_names=["x0", "x2", "x3"]), os_prior),
        "product": ProductKernel([MaternKernel(2.5, GammaPrior(3, 1)), ScaleKernel(RBFKernel(GammaPrior(3, 1)), os_prior)]),
    }[name]


@dataclass
class FitCase:
    tag: str
    n: int
    d: int = 8                  # numerical columns
    kernel: str | None = None   # None: the preset's own kernel
    preset: str = "BAYBE"
    criterion: str = "mll"
    rows: tuple | None = None   # multi-task: training rows per task (T = len(rows), sum = n)
    variants: tuple = ("1",)
    seed: int = 0

    @property
    def id(self):
        return f"{self.tag}-n{self.n}"

    @property
    def T(self):
        return 1 if self.rows is None else len(self.rows)

    @property
    def np_(self):
        return 64 * ((self.n + 63) // 64)

    # ---- the problem ------------------------------------------------------------------------------
    def problem(self):
        """(spec, X_train, y, points): three seeded parameter points, perturbations of ``initial_params`` as the existing tests draw
        them; the third has the noise at the preset's lower bound (conditioning)."""
        from baybe_amd import gp_spec
        from baybe_amd.kernels import apply_kernel_spec

        d, seed = self.d, 1000 * self.n + self.seed
        if self.T == 1:
            _, Xt, y = make_problem(max(4096, 2 * self.n), d, self.n, seed=seed)
            spec = gp_spec.from_preset(self.preset, d, np.zeros(d), np.ones(d))
        else:
            rng = np.random.default_rng(seed)
            parts, ys = [], []
            for t, m in enumerate(self.rows):
                xt = rng.integers(0, 11, size=(m, d)) / 10.0
                yt = -((xt - 0.5) ** 2).sum(1) + 0.1 * np.sin(2 * np.pi * xt[:, 0])
                ys.append((1 - 0.1 * t) * yt + 0.2 * t + 0.05 * rng.standard_normal(m))
                parts.append(np.hstack([xt, np.full((m, 1), float(t))]))
            Xt, y = np.vstack(parts), np.concatenate(ys)
            spec = gp_spec.from_preset(self.preset, d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=self.T)
        spec.criterion = self.criterion
        if self.kernel is not None:
            apply_kernel_spec(spec, _kernel(self.kernel), _space(d))
        bounds = gp_spec.raw_bounds(spec)
        free = np.array([not (b[0] is not None and b[0] == b[1]) for b in bounds])
        lower = np.array([-np.inf if b[0] is None else b[0] for b in bounds])
        p0 = gp_spec.initial_params(spec)
        raw0 = gp_spec.pack_raw(spec, p0)
        nz = np.atleast_1d(p0.noise).size  # (noise slots lead the raw vector: one, or one per task)
        rng = np.random.default_rng(seed + 7)
        points = []
        for k in range(3):
            raw = np.where(free, raw0 + 0.3 * rng.standard_normal(raw0.shape), raw0)
            raw[:nz] = np.abs(raw[:nz]) + 0.01
            raw = np.where(free, np.maximum(raw, 2.0 * lower), raw)  # (box-constrained natural values stay inside their box)
            # the noise at the preset's lower bound, 1e-4 (softplus-constrained: 1e-4 + softplus(-9) = 2.2e-4); not under the dot-product
            # kernels, whose Gram matrix has rank <= 28 here: there the fp64 oracle itself does not resolve the tolerance
            if k == 2 and self.kernel not in ("linear", "poly"):
                raw[0] = bounds[0][0] if bounds[0][0] is not None else -9.0
            points.append(gp_spec.unpack_raw(spec, raw))
        return spec, Xt, y, points

    def analytic(self, spec):
        """The oracle's analytic data term covers this model (kernels on all columns, no dot-product / periodic kernel, one
        likelihood for all tasks); otherwise the comparison goes through the autograd objective."""
        return not (spec.has_subsets or spec.hadamard or spec.has_periodic or self.kernel in ("linear", "poly"))

    # ---- the path this case is built for ----------------------------------------------------------
    def eligible(self, spec):
        from baybe_amd import gp_spec

        tl = len(gp_spec.theta_from_params(spec, gp_spec.initial_params(spec)))
        return (spec.n_factors <= 1 and not spec.hadamard and spec.dn <= 32 and self.T <= 4 and tl <= 49
                and not spec.has_periodic)

    def expected_forms(self, spec, variant):
        """Forms the evaluation may report under ``variant``: one, except where co-residency on the device decides."""
        np_, nbk, elig = self.np_, self.np_ // 64, self.eligible(spec)
        if np_ == 64:
            small = variant != "small0" and self.T == 1 and spec.n_factors <= 1 and self.criterion == "mll" and not spec.hadamard
            return {"small"} if small and not spec.has_periodic else {"launch"}
        if not elig or variant == "0" or np_ > 2048:
            return {"launch"}
        if np_ > 1024:
            return {"one-launch"}
        if variant == "2":
            return {"one-launch"}
        if variant == "3":
            return {"split"}
        if variant == "1-gram0":
            return {"gram+tiles"}
        if variant == "1-steps":
            return {"steps+tail"}
        if variant == "1-mt0":
            return {"tiles"}
        if nbk <= MT_SURE_NBK:
            return {"tiles+mt"}
        return {"tiles+mt", "tiles+mt-partial"} if variant == "1-mtp" else {"tiles+mt", "tiles"}


def _sizes():
    cases = []
    for n in (2, 17, 63, 64):
        cases.append(FitCase("baybe", n, d=5, variants=("small1", "small0")))
    for n in (65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024):
        cases.append(FitCase("baybe", n, variants=ALL_VARIANTS_UP_TO_1024))
    for n in (1025, 1087, 1088, 2047, 2048):
        cases.append(FitCase("baybe", n, variants=("0", "1")))
    for n in (2049, 2100):
        cases.append(FitCase("baybe", n, variants=("1",)))
    return cases


def _models():
    cases = []
    for n in (200, 1088):
        for k in ("m12", "m32", "rbf", "rq", "pp0", "pp2", "linear", "poly", "periodic", "subset", "product"):
            cases.append(FitCase(k, n, d=4 if k == "periodic" else 6, kernel=k, variants=("0", "1")))
        cases.append(FitCase("botorch-mt", n, d=5, preset="BOTORCH", rows=(n // 2, n - n // 2 - n // 5, n // 5), variants=("1",)))
        cases.append(FitCase("icm-loo", n, d=6, criterion="loo", rows=(n // 2, n - n // 2 - n // 6 - n // 9, n // 6, n // 9), variants=("0", "1")))
        cases.append(FitCase("icm-mll", n, d=6, rows=(n - n // 3, n // 3), variants=("0", "1")))
        cases.append(FitCase("icm-mll3", n, d=6, rows=(n // 2, n // 3, n - n // 2 - n // 3), variants=("0", "1")))
        cases.append(FitCase("icm5", n, d=6, criterion="loo", rows=tuple(n // 5 + (t < n % 5) for t in range(5)), variants=("1",)))
        cases.append(FitCase("dn32", n, d=32, variants=("0", "1")))
        cases.append(FitCase("dn33", n, d=33, variants=("1",)))
        cases.append(FitCase("tl49", n, d=30, criterion="loo", rows=(n // 4,) * 3 + (n - 3 * (n // 4),), variants=("0", "1")))
        cases.append(FitCase("tl50", n, d=31, criterion="loo", rows=(n // 4,) * 3 + (n - 3 * (n // 4),), variants=("1",)))
    return cases


CASES = _sizes() + _models()


# ---- the oracle side ----------------------------------------------------------------------------------
def oracle_inputs(spec, Xt, y):
    from oracle import gp_oracle as go

    ospec = oracle_spec(spec)
    return ospec, go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]


def gref_of(spec, dt):
    """The oracle's data-term gradient in the device's theta layout."""
    parts = [[dt.g_noise, dt.g_mean, dt.g_outputscale]]
    parts += (list(dt.g_member_ls) + [dt.g_member_scale]) if spec.factors else [dt.g_ls]
    if spec.n_tasks > 1:  # (theta: head, first kernel's lengthscales, task covariance, the other factors' slots)
        parts.insert(2, dt.g_task_B.reshape(-1))
    if spec.has_rq:
        parts.append(dt.g_alpha)
    return np.concatenate([np.atleast_1d(np.asarray(a, dtype=float)) for a in parts])


def oracle_reference(case, spec, p, ospec, Xn, ys):
    """('analytic', value, gradient in theta layout) or ('autograd', objective, raw gradient) of the oracle at p."""
    from oracle import gp_oracle as go

    if case.analytic(spec):
        dt = go.data_term(ospec, oracle_params(spec, p), Xn, ys)
        return "analytic", dt.value, gref_of(spec, dt)
    f, g = go.fit_objective(ospec, go.pack_raw(ospec, oracle_params(spec, p)), Xn, ys)
    return "autograd", f, np.asarray(g, dtype=float)


def device_in_reference_terms(kind, spec, p, n, val, g):
    """The device's (value, theta gradient) as the quantity the reference gives: itself, or through the host's chain rules the
    objective and its gradient over the free raw slots."""
    from baybe_amd import gp_spec

    if kind == "analytic":
        return val, g
    raw = gp_spec.pack_raw(spec, p)
    f, gr = gp_spec.objective_from_data_term(spec, raw, n, val, g)
    bounds = gp_spec.raw_bounds(spec)
    free = np.array([not (b[0] is not None and b[0] == b[1]) for b in bounds])
    return f, np.asarray(gr, dtype=float)[free]


def tolerances(kind, value, grad):
    """(value tolerance, per-slot gradient tolerances) the device is held to against this reference."""
    gmax = float(np.abs(grad).max()) if grad.size else 0.0
    if kind == "analytic":
        return max(VALUE_RTOL * abs(value), VALUE_ATOL), GRAD_RTOL * np.abs(grad) + GRAD_ATOL_OF_MAX * gmax
    return OBJ_RTOL * abs(value), OBJ_GRAD_RTOL * np.abs(grad) + OBJ_GRAD_ATOL_OF_MAX * gmax


def mismatch(kind, ref_val, ref_grad, val, grad):
    """Largest ratio |deviation| / tolerance over the value and every gradient slot (<= 1: within tolerance)."""
    tv, tg = tolerances(kind, ref_val, ref_grad)
    return max(abs(val - ref_val) / tv, float(np.max(np.abs(np.asarray(grad) - ref_grad) / tg)) if ref_grad.size else 0.0)

