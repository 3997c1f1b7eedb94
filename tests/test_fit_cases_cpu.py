"""The case table of tests/test_fit_forms_gpu.py checked with the oracle alone, for every row:

(a) the reference is far below the tolerance: its own value / gradient spread under a permutation of the training rows is at most
    1/100 of what the device is allowed;
(b) the tolerance would catch a padding-class bug: one extra identity-like pad row with target 0 (a row far outside the inputs,
    uncorrelated with the others), and separately the last real row dropped, each move some checked quantity by >= 100 times its
    tolerance."""

import numpy as np
import pytest

from _fit_cases import CASES, mismatch, oracle_inputs, oracle_reference, tolerances

# rows that differ only in their switches share one problem
_PROBLEMS = {}
for _c in CASES:
    _PROBLEMS.setdefault((_c.tag, _c.n, _c.d, _c.kernel, _c.preset, _c.criterion, _c.rows), _c)
ROWS = list(_PROBLEMS.values())


def _pad_row(spec, case, Xn):
    row = Xn[:1].copy()
    num = np.asarray(spec.num_idx)
    # stationary kernels: far away, so its kernel row is 0 off the diagonal; dot-product kernels: the origin
    row[0, num] = 0.0 if case.kernel in ("linear", "poly") else 1e3
    return row


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_oracle_resolves_the_device_tolerance(case):
    spec, Xt, y, points = case.problem()
    ospec, Xn, ys = oracle_inputs(spec, Xt, y)
    p = points[2]  # (the least well-conditioned point: noise at its lower bound)
    kind, v, g = oracle_reference(case, spec, p, ospec, Xn, ys)
    tv, tg = tolerances(kind, v, g)
    # (a) the oracle's own rounding
    perm = np.random.default_rng(case.n).permutation(case.n)
    _, vp, gp = oracle_reference(case, spec, p, ospec, Xn[perm], ys[perm])
    spread = mismatch(kind, v, g, vp, gp)
    assert spread <= 1e-2, (case.id, "permutation spread / tolerance", spread)
    # (b) a padding-class bug moves a checked quantity by >= 100 tolerances
    Xpad = np.vstack([Xn, _pad_row(spec, case, Xn)])
    _, va, ga = oracle_reference(case, spec, p, ospec, Xpad, np.append(ys, 0.0))
    assert mismatch(kind, v, g, va, ga) >= 100.0, (case.id, "pad row", mismatch(kind, v, g, va, ga))
    if case.n > 1:
        _, vd, gd = oracle_reference(case, spec, p, ospec, Xn[:-1], ys[:-1])
        assert mismatch(kind, v, g, vd, gd) >= 100.0, (case.id, "last row dropped", mismatch(kind, v, g, vd, gd))
