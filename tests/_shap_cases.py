"""TEST INFRASTRUCTURE - shared fixtures of the Shapley tests (tests/test_shap_cpu.py guards them, tests/test_shap_gpu.py runs them).

Models have hand-set hyper-parameters and a standardised noise of ``max(0.01, n / 8000)`` (tests/_nipv_cases.py: with a kernel
value of at most ``kmax`` the condition number of ``K + s2 I`` stays below ``kmax n / noise + 1``), so that a deviation beyond the
bound stays interpretable.

Shapes (the issue's table): the smallest legal call; n no multiple of the 16-point table block; M = 5 with an uneven low / high
split (3 + 2), a one-hot group of three columns and a column in no group, R = 17 and B = 33 off any tile width, for each of the four
kernels with and without outputscale; M = 16, the largest mask; n = 512, the limit; and M = 10 for the four-coalitions-per-thread
instantiation (``BBH_SHAP_CPT=4`` needs 1024 coalitions).  Special rows, where a case has room: explained row 0 IS background row 0,
row 1 IS training row 0 (the 1e-30 clamp), the last row repeats row 3 (R >= 17)."""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

MAX_FEATURES = 16
C_START = 1.0  # the constant the issue starts from
C_BOUND = 0.5  # shipped: the largest observed |device - oracle| / tol(c = 1), 0.074, rounded up to the next power of two (0.125), times 4 (profiles/shap_observed_deviations.json)
KINDS = ("matern12", "matern32", "matern52", "rbf")


class Case:
    def __init__(self, name, kernel, M, R, B, n, groups, scale=False, seed=0, model="single"):
        self.id, self.kernel, self.M, self.R, self.B, self.n = name, kernel, M, R, B, n
        self.groups = np.asarray(groups, dtype=np.int32)
        self.d = len(self.groups)
        self.scale, self.seed, self.model = bool(scale), seed, model

    # ---- the model on the device's side and on the oracle's --------------------------------------------------------------------
    def device_spec(self):
        """(GPSpec, GPParams) of ``baybe_amd.gp_spec``."""
        from baybe_amd import gp_spec

        c = self.build()
        d = self.d
        if self.model == "icm":  # two tasks, INT-coded in the last column
            spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d), task_idx=d - 1, n_tasks=2, kernel=self.kernel)
        elif self.model == "composite":
            from baybe_amd.kernels import MaternKernel, ProductKernel, RBFKernel, ScaleKernel, apply_kernel_spec

            spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
            apply_kernel_spec(spec, ProductKernel([MaternKernel(2.5), ScaleKernel(RBFKernel())]))
        else:
            spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d), kernel=self.kernel)
            spec.use_outputscale = self.scale
        p = gp_spec.initial_params(spec)
        p.lengthscale = np.array(c.ls)
        p.noise, p.mean = c.noise, 0.1
        if self.model == "composite":
            p.lengthscale = np.array(c.ls) * np.sqrt(2.0)
            p.factor_ls = [np.array(c.ls2) * np.sqrt(2.0)]
            p.factor_os = np.array([1.0, 1.3])
        elif self.model == "icm":
            p.task_W = np.array(c.task_W)
            p.task_v = np.array(c.task_v)
        elif self.scale:
            p.outputscale = 1.7
        return spec, p

    @functools.lru_cache(maxsize=None)
    def build(self):
        rng = np.random.default_rng([self.seed, self.M, self.R, self.B, self.n, self.d])
        d, dnum = self.d, self.d - (1 if self.model == "icm" else 0)
        Xt, Bg, X = rng.random((self.n, d)), rng.random((self.B, d)), rng.random((self.R, d))
        if self.model == "icm":
            Xt[:, -1], Bg[:, -1], X[:, -1] = rng.integers(0, 2, self.n), rng.integers(0, 2, self.B), rng.integers(0, 2, self.R)
            Xt[:2, -1] = (0.0, 1.0)
        if self.R >= 2:
            X[0] = Bg[0]
            X[1] = Xt[0]
        if self.R >= 17:
            X[-1] = X[3]
        u = Xt[:, :dnum]
        y = np.sin(3.0 * u.sum(axis=1) / np.sqrt(dnum)) + 0.3 * u[:, 0] + 0.05 * rng.standard_normal(self.n) + 0.2 * Xt[:, -1]
        ls = 0.35 * np.sqrt(dnum) * (1.0 + 0.3 * rng.random(dnum))
        ls2 = 0.5 * np.sqrt(dnum) * (1.0 + 0.3 * rng.random(dnum))
        noise = max(0.01, self.n / 8000.0)
        out = SimpleNamespace(Xt=Xt, y=y, Bg=Bg, X=X, ls=ls, ls2=ls2, noise=noise, task_W=0.3 + rng.random((2, 2)), task_v=0.5 + rng.random(2))
        for a in vars(out).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def oracle_model(self):
        from _problems import oracle_params, oracle_spec
        from oracle import gp_oracle as go

        c = self.build()
        spec, p = self.device_spec()
        return go.fit_gp(oracle_spec(spec), np.array(c.Xt), np.array(c.y), oracle_params(spec, p))

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """The oracle's v, phi, base and the bound at c = 1, computed once and shared."""
        import _oracle_shap as osh

        c = self.build()
        ref = osh.explain(self.oracle_model(), np.array(c.X), np.array(c.Bg), self.groups, self.M)
        for a in vars(ref).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return ref


ONE_HOT = (0, 1, 1, 1, 2, -1, 3, 4)  # five features over eight columns: one group of three one-hot columns, one column in no group
CASES = (
    [Case("smallest", "matern52", 1, 1, 1, 1, (0,)),
     Case("n17", "matern32", 2, 1, 3, 17, (0, 1))]
    + [Case(f"m5-{k}{'-os' if s else ''}", k, 5, 17, 33, 64, ONE_HOT, scale=s, seed=3) for k in KINDS for s in (False, True)]
    + [Case("m16", "matern52", 16, 1, 2, 3, tuple(range(16))),
       Case("n512", "rbf", 3, 2, 3, 512, (0, 1, 2)),
       Case("m10", "matern52", 10, 2, 2, 5, tuple(range(10)))]
)
BY_ID = {c.id: c for c in CASES}
REPRO_CASE = BY_ID["m5-matern52"]
CPT_CASE = BY_ID["m10"]
# models the fused form refuses and form="auto" answers through the composed one (M = 3, R = 2, B = 3)
COMPOSITE_CASE = Case("composite", "matern52", 3, 2, 3, 20, (0, 1, 2), seed=5, model="composite")
ICM_CASE = Case("icm", "matern52", 3, 2, 3, 20, (0, 1, 2), seed=6, model="icm")  # the task column is feature 2
OVER_N_CASE = Case("n513", "matern52", 3, 2, 3, 513, (0, 1, 2), seed=7)


# ---- a stub search space with a categorical parameter (tests/_baybe_shim.py has numerical parameters only) ------------------------
class CategoricalParameter:
    """One-hot encoded: the comp-rep columns ``<name>_<value>``."""

    is_numerical, is_discrete, is_continuous = False, True, False

    def __init__(self, name, values):
        self.name, self.values = name, tuple(values)


class NumericalParameter:
    is_numerical, is_discrete, is_continuous = True, True, False

    def __init__(self, name, values):
        self.name, self.values = name, tuple(float(v) for v in values)


class _NoContinuous:
    is_empty = True


class StubSpace:
    """What the surrogates and ``baybe_amd.insights`` read of a search space: ``parameters``, ``comp_rep_columns``,
    ``get_comp_rep_parameter_indices``, ``scaling_bounds``, ``transform``; no task parameter."""

    task_idx, n_tasks = None, 1

    def __init__(self, parameters, with_indices=True, extra_columns=()):
        self.parameters = tuple(parameters)
        self.continuous = _NoContinuous()
        self._extra = tuple(extra_columns)  # comp-rep columns no parameter owns (only for the group-construction test)
        if with_indices:
            self.get_comp_rep_parameter_indices = self._indices

    def _cols_of(self, p):
        return [p.name] if p.is_numerical else [f"{p.name}_{v}" for v in p.values]

    @property
    def comp_rep_columns(self):
        return tuple(c for p in self.parameters for c in self._cols_of(p)) + self._extra

    def _indices(self, name):
        cols = self.comp_rep_columns
        p = {q.name: q for q in self.parameters}[name]
        return tuple(cols.index(c) for c in self._cols_of(p))

    @property
    def scaling_bounds(self):
        import pandas as pd

        lo, hi = [], []
        for p in self.parameters:
            for _ in self._cols_of(p):
                lo.append(min(p.values) if p.is_numerical else 0.0), hi.append(max(p.values) if p.is_numerical else 1.0)
        lo, hi = lo + [0.0] * len(self._extra), hi + [1.0] * len(self._extra)
        return pd.DataFrame([lo, hi], index=["min", "max"], columns=self.comp_rep_columns)

    def transform(self, df, allow_extra=False):
        import pandas as pd

        out = pd.DataFrame(index=df.index)
        for p in self.parameters:
            if p.is_numerical:
                out[p.name] = df[p.name].astype(float)
            else:
                for v in p.values:
                    out[f"{p.name}_{v}"] = (df[p.name] == v).astype(float)
        for c in self._extra:
            out[c] = 0.0
        return out


def surface_problem(two_targets: bool = False):
    """(space, measurements, objective): one numerical and one three-level categorical parameter, 12 measured rows."""
    import pandas as pd
    from _baybe_shim import NumericalTarget, ParetoObjective, SingleTargetObjective

    rng = np.random.default_rng(21)
    space = StubSpace([NumericalParameter("x", np.linspace(0.0, 1.0, 6)), CategoricalParameter("c", ("a", "b", "c"))])
    x = rng.choice(np.linspace(0.0, 1.0, 6), 12)
    c = rng.choice(["a", "b", "c"], 12)
    off = pd.Series(c).map({"a": 0.0, "b": 0.5, "c": -0.4}).to_numpy()
    meas = pd.DataFrame({"x": x, "c": c, "t": np.sin(3.0 * x) + off + 0.02 * rng.standard_normal(12),
                         "u": (x - 0.3) ** 2 - off + 0.02 * rng.standard_normal(12)})
    if two_targets:
        return space, meas, ParetoObjective([NumericalTarget("t"), NumericalTarget("u", minimize=True)])
    return space, meas, SingleTargetObjective(NumericalTarget("t"))
