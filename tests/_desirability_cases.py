"""Descriptions, inputs and stand-in objects shared by tests/test_desirability_cpu.py (which guards the cases) and
tests/test_desirability_gpu.py (which runs them on the device).

Targets are built from ``_objective_cases.PROGRAMS`` and variations of them; the sets for the geometric mean have images in
[0, 1] (what the reference demands of normalised targets), the sets for the arithmetic mean also hold programs with images beyond
it.  Per-target joint statistics come from ``_joint_cases.JointCase``: one case per target, different seeds of the mean families 0
and 3, so every target has its own candidates' means, variances, cross-covariances and pending statistics; target t's rows are rolled
by t positions, so the regimes (ordinary / jitter / notpd) of one row differ between the targets.  The mask is shared."""

from __future__ import annotations

import functools

import numpy as np

import _objective_cases as oc
import _oracle_desirability as od
from _joint_cases import JointCase

P = oc.PROGRAMS
_RAMP_MIN = (("AFFINE", (-0.4, 0.6)), ("CLAMP", (0.0, 1.0)), ("AFFINE", (-1.0, 1.0)))  # a minimised normalised ramp: 1 - ramp
_BELL2 = (("BELL", (-0.5, 1.2)),)
_BELL3 = (("BELL", (1.0, 2.0)),)
_RAMP2 = (("AFFINE", (0.25, 0.5)), ("CLAMP", (0.0, 1.0)))
_SIGMOID2 = (("SIGMOID", (-0.3, -0.9)),)
_UNIT = {2: (P["bell"], P["ramp"]), 3: (P["sigmoid"], P["bell"], P["ramp"]),
         8: (P["bell"], P["ramp"], P["sigmoid"], _BELL2, _RAMP2, _SIGMOID2, _RAMP_MIN, _BELL3)}
_BEYOND = {2: (P["power3-min"], P["bell"]), 3: (P["clamp-log"], P["ramp"], P["triangular-min"]),
           8: (P["bell"], P["triangular-min"], P["sigmoid"], _BELL2, P["clamp-log"], _SIGMOID2, _RAMP_MIN, P["power3-min"])}
_RAW_WEIGHTS = {2: (2.0, 1.0), 3: (1.0, 2.5, 1.5), 8: (1.0, 2.0, 0.5, 1.5, 1.0, 3.0, 0.75, 1.25)}
TARGET_COUNTS = (2, 3, 8)
SCALARIZERS = ("GEOM_MEAN", "MEAN")
BETA = oc.BETA
MC_KINDS = oc.MC_KINDS


def description(T: int, scalarizer: str) -> od.Des:
    w = np.asarray(_RAW_WEIGHTS[T])
    return od.Des((_UNIT if scalarizer == "GEOM_MEAN" else _BEYOND)[T], tuple(w / w.sum()), scalarizer)


def product_program(des: od.Des):
    """The product's ``DesirabilityProgram`` of an oracle description (the GPU module hands it to ``HipGP.desirability_acq``)."""
    from baybe_amd.desirability import DesirabilityProgram
    from baybe_amd.objective import ObjectiveProgram

    return DesirabilityProgram(tuple(ObjectiveProgram(tuple(ops)) for ops in des.programs), tuple(des.weights), des.scalarizer)


def case_best_f(des: od.Des, mean) -> float:
    """The incumbent of a synthetic case: the 70 % quantile of the desirability of the candidates' means [T, N]."""
    return float(np.quantile(od.desirability(des, np.moveaxis(np.asarray(mean), 0, -1)), 0.7))


# ---- q' = 1 ---------------------------------------------------------------------------------------------------------------------
Q1_SHAPES = oc.Q1_SHAPES  # N in (1, 257) x S in (1, 33, 512)


@functools.lru_cache(maxsize=None)
def q1_inputs(N, S, T):
    """(mean [T, N], var [T, N], z [S, T], alive [N]): at N = 257 rows 3 and 5 need the 1 x 1 jitter in some targets, row 100 is
    masked."""
    from oracle import gp_oracle as go

    rng = np.random.default_rng([N, S, T])
    mean, var = rng.standard_normal((T, N)), 0.05 + 0.5 * rng.random((T, N))
    alive = np.ones(N, dtype=np.uint8)
    if N > 100:
        var[0, 3], var[T - 1, 5], var[1, 5], alive[100] = 0.0, -1e-9, -3e-8, 0
    z = go.sobol_normal_base_samples(S, T, 7).copy()
    for a in (mean, var, z, alive):
        a.setflags(write=False)
    return mean, var, z, alive


# ---- joint ------------------------------------------------------------------------------------------------------------------------
# seeds of the mean families 0 and 3, one per target.  A (case, scalariser, kind) that misses the guard of
# tests/test_desirability_cpu.py is reseeded HERE (next seed of the same family), never loosened on the device.
_SEEDS = (0, 3, 4, 7, 8, 11, 12, 15)
_RESEEDED: dict = {}  # (T, p, target) -> seed


class JointSet:
    """T ``JointCase`` s of the same (p, S, N) stacked target-major."""

    def __init__(self, T, p, S, N=130, form=0):
        self.T, self.p, self.S, self.N, self.form = T, p, S, N, form  # form: what ``bbh_desirability_last_form`` must report
        self.cases = tuple(JointCase(p, S, N, 1.0, _RESEEDED.get((T, p, t), _SEEDS[t])) for t in range(T))
        assert all(c.family in (0, 3) for c in self.cases)

    @property
    def id(self):
        return f"T{self.T}-p{self.p}-S{self.S}-N{self.N}"

    def build(self):
        return _build(self.T, self.p, self.S, self.N, self.cases)


class JointSetData:
    """Target t takes its case's rows rolled by t positions, so the regimes of one row differ between the targets: a row scores NaN
    as soon as ANY target's covariance is labelled not-PSD there; the mask is the first target's."""

    def __init__(self, cases, T, p, S):
        from oracle import gp_oracle as go

        ds = [c.build() for c in cases]
        roll = lambda a, t: np.roll(a, t, axis=0)  # noqa: E731
        self.mean, self.var = np.stack([roll(d.mean, t) for t, d in enumerate(ds)]), np.stack([roll(d.var, t) for t, d in enumerate(ds)])
        self.cross = np.stack([roll(d.cross, t) for t, d in enumerate(ds)])
        self.mean_p, self.cov_pp = np.stack([d.mean_p for d in ds]), np.stack([d.cov_pp for d in ds])
        self.alive = ds[0].alive
        self.labels = tuple(tuple(np.roll(np.array(d.labels), t)) for t, d in enumerate(ds))  # [T][N]
        self.z = go.sobol_normal_base_samples(S, (p + 1) * T, 5).reshape(S, p + 1, T).copy()
        for a in (self.mean, self.var, self.cross, self.mean_p, self.cov_pp, self.z):
            a.setflags(write=False)

    def target_is_label(self, t, *names):
        return np.array([lab in names for lab in self.labels[t]])

    @property
    def masked(self):
        return ~self.alive.astype(bool)

    @property
    def notpd(self):
        """Live rows of which at least one target's covariance does not factor."""
        return np.any([self.target_is_label(t, "notpd") for t in range(len(self.labels))], axis=0) & ~self.masked

    @property
    def scored(self):
        return ~self.masked & ~self.notpd

    def sigmas(self):
        """[T, N, q, q] joint covariances and [T, N, q] joint means."""
        Sig = np.stack([od.sigma(self.var[t], self.cross[t], self.cov_pp[t]) for t in range(len(self.mean))])
        return Sig, od.joint_means(self.mean, self.mean_p)


@functools.lru_cache(maxsize=None)
def _build(T, p, S, N, cases):
    return JointSetData(cases, T, p, S)


# N = 130: two full 64-thread workgroups and a ragged one.  (2, 15): the LDS form at its largest; (8, 15): the factors do not fit
# the LDS, the workspace form.
JOINT_SETS = (JointSet(2, 15, 33), JointSet(3, 1, 128), JointSet(8, 2, 33), JointSet(8, 15, 33, form=1), JointSet(3, 5, 100, N=1))
FORM_SETS = (JointSet(2, 1, 33), JointSet(3, 4, 33))  # both forms legal: bit-for-bit equality
AGREE_P = (0, 4, 15)


def compare_rows(got, d: JointSetData, ident: str):
    """NaN rows are exactly the live rows that are notpd in some target, -inf rows exactly the masked rows, every other row is finite."""
    got = np.asarray(got)
    assert np.array_equal(np.isnan(got), d.notpd), (ident, "NaN rows")
    assert np.array_equal(np.isneginf(got), d.masked), (ident, "-inf rows")
    assert np.isfinite(got[d.scored]).all(), (ident, "non-finite score of a live row")


# ---- stand-ins for the reference's objects (recognised by attribute, like the real ones) -------------------------------------------
class DesirabilityObjective:
    """What the product reads of ``baybe.objectives.DesirabilityObjective(as_pre_transformation=False)``."""

    is_multi_output = False
    as_pre_transformation = False

    def __init__(self, targets, weights=None, scalarizer="GEOM_MEAN"):
        self.targets = tuple(targets)
        self.weights = tuple(1.0 for _ in self.targets) if weights is None else tuple(float(w) for w in weights)
        self.scalarizer = scalarizer

    @property
    def _modeled_quantities(self):
        return self.targets

    @property
    def _model_quantities_to_target_names(self):
        return {t.name: [t.name] for t in self.targets}

    @property
    def normalized_weights(self):
        w = np.asarray(self.weights)
        return tuple(w / w.sum())


def ramp_target(name, lo, hi, descending=False):
    """``NumericalTarget.normalized_ramp(name, (lo, hi), descending)``: an affine map onto [0, 1], clamped."""
    a = 1.0 / (hi - lo)
    affine = oc._tr("AffineTransformation", factor=-a, shift=hi * a) if descending else oc._tr("AffineTransformation", factor=a, shift=-lo * a)
    cut = type("Interval", (), {"lower": 0.0, "upper": 1.0})()
    chain = oc._tr("ChainedTransformation", transformations=(affine, oc._tr("ClampingTransformation", cutoffs=cut)))
    return oc._Target(name, chain, False)
