"""Objective programs: a single target's transformation as a short list of scalar operations.

In the reference the surrogate is fitted on the raw target and the target's ``transformation`` acts per posterior sample, as an MC
objective in front of the acquisition utility (``acquisition/_builder.py:211-254``, ``objectives/base.py:130-150``,
``transformations/basic.py``); minimisation appends a negation (``_oriented_targets``, ``objectives/base.py:100-105``).  Here the
transformation is walked once on the host into at most ``MAX_OPS`` operations, which the acquisition kernels of
``csrc/bbh_objacq.hip`` evaluate in registers between the joint draw and the utility (``bbh_apply_objective``, csrc/bbh_objective.h).
The classes are recognised by name, like ``kernels.apply_kernel_spec`` does, so the module needs no import of BayBE.

``ObjectiveProgram.apply`` is the numpy interpreter of the same list; the host uses it for ``best_f`` (the "transformed posterior
mean" of ``_builder.py:141-161``)."""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from baybe_amd.exceptions import IncompatibilityError

MAX_OPS = 8  # bbh_objective_prog holds 8 operations
# operation -> (code of ``enum bbh_objective_op``, number of parameters)
OPS = {"AFFINE": (0, 2), "CLAMP": (1, 2), "TWOSIDED": (2, 3), "BELL": (3, 2), "LOG": (4, 0), "EXP": (5, 0), "POW": (6, 1),
       "SIGMOID": (7, 2)}
_REFUSED = ("CustomTransformation", "AdditiveTransformation", "MultiplicativeTransformation")


@dataclass(frozen=True)
class ObjectiveProgram:
    """``ops``: tuple of (operation name, parameters), applied first to last."""

    ops: tuple

    def apply(self, x: np.ndarray) -> np.ndarray:
        y = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            for op, p in self.ops:
                if op == "AFFINE":
                    y = y * p[0] + p[1]
                elif op == "CLAMP":
                    y = np.minimum(np.maximum(y, p[0]), p[1])
                elif op == "TWOSIDED":
                    y = np.where(y < p[2], (y - p[2]) * p[0], (y - p[2]) * p[1])
                elif op == "BELL":
                    y = np.exp(-(((y - p[0]) / p[1]) ** 2.0) / 2.0)
                elif op == "LOG":
                    y = np.log(y)
                elif op == "EXP":
                    y = np.exp(y)
                elif op == "POW":
                    y = np.power(y, p[0])
                elif op == "SIGMOID":
                    y = 1.0 / (1.0 + np.exp(p[1] * (y - p[0])))
                else:  # pragma: no cover
                    raise ValueError(op)
        return y

    def as_affine(self):
        """(a, b) if the program is one affine map - the case the reference treats as a posterior transform
        (``objectives/single.py:77-91``) - else None."""
        if len(self.ops) == 1 and self.ops[0][0] == "AFFINE":
            return self.ops[0][1]
        return None

    def to_struct(self):
        """``bbh_objective_prog`` for the C-ABI."""
        from baybe_amd import _lib

        prog = _lib.ObjectiveProg()
        prog.n_ops = len(self.ops)
        for i, (op, p) in enumerate(self.ops):
            prog.op[i] = OPS[op][0]
            for j, v in enumerate(p):
                prog.p[i][j] = float(v)
        return prog


def _unreadable(tr, what) -> IncompatibilityError:
    return IncompatibilityError(
        f"The parameters of the '{type(tr).__name__}' cannot be read ({what}); the HIP path evaluates target transformations "
        f"from their parameters. Use BotorchRecommender."
    )


def _num(tr, name: str) -> float:
    try:
        v = float(getattr(tr, name))
    except (AttributeError, TypeError, ValueError) as ex:
        raise _unreadable(tr, f"'{name}'") from ex
    if math.isnan(v):
        raise _unreadable(tr, f"'{name}' is NaN")
    return v


def _walk(tr, ops: list) -> None:
    kind = type(tr).__name__
    if kind == "IdentityTransformation":
        return
    if kind in _REFUSED:
        raise IncompatibilityError(
            f"A '{kind}' is not expressible as a chain of scalar operations; the HIP path supports chains of affine, clamping, "
            f"two-sided affine, bell, logarithmic, exponential, integer power and sigmoid transformations. Use BotorchRecommender."
        )
    if kind == "ChainedTransformation":
        try:
            members = tuple(tr.transformations)
        except (AttributeError, TypeError) as ex:
            raise _unreadable(tr, "'transformations'") from ex
        for t in members:
            _walk(t, ops)
    elif kind in ("AbsoluteTransformation", "TriangularTransformation"):
        inner = getattr(tr, "_transformation", None)
        if inner is None:
            raise _unreadable(tr, "'_transformation'")
        _walk(inner, ops)
    elif kind == "AffineTransformation":
        ops.append(("AFFINE", (_num(tr, "factor"), _num(tr, "shift"))))
    elif kind == "ClampingTransformation":
        cut = getattr(tr, "cutoffs", None)
        if cut is None:
            raise _unreadable(tr, "'cutoffs'")
        ops.append(("CLAMP", (_num(cut, "lower"), _num(cut, "upper"))))
    elif kind == "TwoSidedAffineTransformation":
        ops.append(("TWOSIDED", (_num(tr, "slope_left"), _num(tr, "slope_right"), _num(tr, "midpoint"))))
    elif kind == "BellTransformation":
        ops.append(("BELL", (_num(tr, "center"), _num(tr, "sigma"))))
    elif kind == "LogarithmicTransformation":
        ops.append(("LOG", ()))
    elif kind == "ExponentialTransformation":
        ops.append(("EXP", ()))
    elif kind == "PowerTransformation":
        e = _num(tr, "exponent")
        if e != int(e) or abs(e) > 2**31 - 1:
            # (the reference raises for a negative sample under a non-integer exponent - data-dependently, transformations/basic.py:437-443)
            raise IncompatibilityError(
                f"The 'PowerTransformation' has the non-integer exponent {e}; posterior samples take either sign, so the HIP path "
                f"supports integer exponents only. Use BotorchRecommender."
            )
        ops.append(("POW", (e,)))
    elif kind == "SigmoidTransformation":
        ops.append(("SIGMOID", (_num(tr, "center"), _num(tr, "steepness"))))
    else:
        raise IncompatibilityError(
            f"Transformations of type '{kind}' are not on the HIP path. Use BotorchRecommender."
        )


def _fold(ops: list) -> list:
    """Adjacent affine maps become one; an identity map among other operations is dropped."""
    out: list = []
    for op, p in ops:
        if op == "AFFINE" and out and out[-1][0] == "AFFINE":
            a1, b1 = out[-1][1]
            out[-1] = ("AFFINE", (p[0] * a1, p[0] * b1 + p[1]))
        else:
            out.append((op, tuple(p)))
    kept = [o for o in out if not (o[0] == "AFFINE" and o[1] == (1.0, 0.0))]
    return kept if kept else [("AFFINE", (1.0, 0.0))]


def objective_program(target) -> ObjectiveProgram | None:
    """The program of a ``NumericalTarget``: its transformation, then a negation if it is minimised.  None for an identity
    transformation, minimised or not: those targets stay on the ``sign`` path of the kernels."""
    tr = getattr(target, "transformation", None)
    if tr is None or type(tr).__name__ == "IdentityTransformation":
        return None
    ops: list = []
    _walk(tr, ops)
    if getattr(target, "minimize", False):
        ops.append(("AFFINE", (-1.0, 0.0)))
    ops = _fold(ops)
    if len(ops) > MAX_OPS:
        raise IncompatibilityError(
            f"The '{type(tr).__name__}' of target '{getattr(target, 'name', '?')}' needs {len(ops)} operations after folding; the "
            f"HIP kernels evaluate at most {MAX_OPS}. Use BotorchRecommender."
        )
    return ObjectiveProgram(tuple(ops))
