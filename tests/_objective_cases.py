"""Programs, inputs and stand-in targets shared by tests/test_objective_cpu.py (which guards the cases) and
tests/test_objective_gpu.py (which runs them on the device).  Programs are written out as operation lists - what
``baybe_amd.objective.objective_program`` produces for the named constructors of the reference (tests/test_objective_cpu.py pins
that where the reference is importable) - so that the GPU module needs nothing but numpy."""

from __future__ import annotations

import numpy as np

from _joint_cases import ONE_ROW_CASE, JointCase

INF = float("inf")
MC_KINDS = ("qLogEI", "qEI", "qPI", "qSR", "qUCB", "qPSTD")
MC_RTOL, MC_ATOL = 1e-8, 1e-9  # tests/test_joint_batch_gpu.py
BETA = 0.4

PROGRAMS = {
    "bell": (("BELL", (0.4, 0.8)),),  # match_bell(0.4, 0.8)
    # match_triangular(0.5, cutoffs=(-1, 2), mismatch_instead=True): two-sided affine + 1, clamp(min=0), negation
    "triangular-min": (("TWOSIDED", (1 / 1.5, -1 / 1.5, 0.5)), ("AFFINE", (1.0, 1.0)), ("CLAMP", (0.0, INF)), ("AFFINE", (-1.0, 0.0))),
    "ramp": (("AFFINE", (-0.4, 0.6)), ("CLAMP", (0.0, 1.0))),  # normalized_ramp((-1, 1.5), descending=True)
    # match_power(0.3, 3): shift, absolute value, cube, negation (minimised)
    "power3-min": (("AFFINE", (1.0, -0.3)), ("TWOSIDED", (-1.0, 1.0, 0.0)), ("POW", (3.0,)), ("AFFINE", (-1.0, 0.0))),
    "clamp-log": (("CLAMP", (0.1, INF)), ("LOG", ())),  # .clamp(min=0.1).log()
    "sigmoid": (("SIGMOID", (0.2, 1.7)),),
}

# 130 rows: two full 64-thread workgroups and a ragged one, every regime of _joint_cases.CYCLE; seeds of mean families 0 and 3 only
# (family 2's 1e-10 covariance scale is meaningless under a bell).  A (case, program, kind) that misses the guard of
# tests/test_objective_cpu.py is reseeded HERE (next seed of the same family), never loosened on the device.
JOINT_CASES = (JointCase(1, 33, 130, 1.0, 0), JointCase(1, 128, 130, 1.0, 3), JointCase(2, 33, 130, 1.0, 3), JointCase(2, 128, 130, 1.0, 0),
               JointCase(15, 33, 130, 1.0, 0), JointCase(15, 128, 130, 1.0, 3), ONE_ROW_CASE)
assert all(c.family in (0, 3) for c in JOINT_CASES)


def case_best_f(ops, mean) -> float:
    """The incumbent of a synthetic case: the 70 % quantile of the program over the candidates' means."""
    from _oracle_objective import apply_program

    return float(np.quantile(apply_program(ops, mean), 0.7))


Q1_SHAPES = [(N, S) for N in (1, 257) for S in (1, 33, 512)]  # one thread; a full 256-thread workgroup and a ragged one


def q1_inputs(N, S):
    """(mean, var, z, alive): rows 3 and 5 need the 1 x 1 jitter, row 100 is masked (N = 257)."""
    from oracle import gp_oracle as go

    rng = np.random.default_rng([N, S])
    mean, var = rng.standard_normal(N), 0.05 + 0.5 * rng.random(N)
    alive = np.ones(N, dtype=np.uint8)
    if N > 100:
        var[3], var[5], alive[100] = 0.0, -1e-9, 0
    return mean, var, go.sobol_normal_base_samples(S, 1, 7)[:, 0].copy(), alive


def mc_ratio(got, ref):
    """Largest |got - ref| in units of the MC tolerance MC_ATOL + MC_RTOL |ref|."""
    return float((np.abs(got - ref) / (MC_ATOL + MC_RTOL * np.abs(ref))).max()) if len(ref) else 0.0


# ---- stand-ins for the reference's transformation classes (recognised by class name, like the real ones) -----------------------
def _tr(name, **attrs):
    return type(name, (), {})() if not attrs else type(name, (), attrs)()


def bell_target(name, center, sigma, minimize=False):
    return _Target(name, _tr("BellTransformation", center=center, sigma=sigma), minimize)


def absolute_target(name, match_value):
    """``NumericalTarget.match_absolute``: shift, absolute value; minimised."""
    inner = _tr("TwoSidedAffineTransformation", slope_left=-1.0, slope_right=1.0, midpoint=0.0)
    chain = _tr("ChainedTransformation", transformations=(_tr("AffineTransformation", factor=1.0, shift=-match_value),
                                                          _tr("AbsoluteTransformation", _transformation=inner)))
    return _Target(name, chain, True)


def affine_target(name, factor, shift, minimize=False):
    return _Target(name, _tr("AffineTransformation", factor=factor, shift=shift), minimize)


class _Target:
    def __init__(self, name, transformation, minimize):
        self.name, self.transformation, self.minimize = name, transformation, minimize
