"""TEST INFRASTRUCTURE - k-medoids cases shared by tests/test_pam_cpu.py and tests/test_pam_gpu.py.

A case is a ``Case``: seeded points, the call's arguments, the seed of the global ``np.random`` generator (or an int
``random_state``), optionally the candidate rows.  Inputs are regenerated from seeds, so the golden file
(tests/golden/pam_reference_medoids.npz) holds only medoid indices.

* generic     seeded standard-normal points with N >= 20 k, held to the oracle AND to the reference's own ``medoid_indices_``.  Why
              N >= 20 k: a two-member cluster is a mathematical tie - cost(a) = cost(b) = dist(a, b) - which the reference resolves
              by the ulp asymmetry of sklearn's |x|^2 + |y|^2 - 2 x.y matrix, and that is no contract; small clusters appear when N / k
              is small.  Shapes: the edges of the 64-row column tile and the 256-row row tile of the cost kernel, d on both sides of
              every register-form width (2, 4, 8, 12, 16, 20, 24, 32) and generic-form widths on both sides of the 96-column LDS
              tile step.
* edge        the sizes below 20 k, held to the oracle only: 1, 2, 3 rows with every k; k = N at 65 rows (every cluster has one member,
              and k crosses the 64-medoid LDS tile of the assignment); wide rows (d = 200, 400, 768: the 16- and 8-column LDS tiles,
              k = 40 across five 8-medoid tiles); 300 rows with k = 150 (many one- and two-member clusters).
* grids       product grids from ``_fps_cases.GRIDS``, standard-scaled: massive exact ties.
* duplicates  duplicated rows; one seed, found on the CPU, for which ``init="random"`` draws two identical rows: the second of the two
              clusters is empty (the warning) - its medoid stays outside its own cluster.
* max_iter    0 (no iteration: the initial medoids) and 1 on an input that needs more (the ConvergenceWarning).
* subset      a candidate subset of a larger resident matrix.
* outlier     one point far away: a one-member cluster next to clusters that straddle row tiles.
* long        16 700 x 2, k = 3: clusters spanning some twenty row tiles each (GPU test only; two iterations).
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

import _fps_cases as fc
import _oracle_pam as oracle


@dataclass
class Case:
    name: str
    make: object  # () -> points [N, d]
    k: int
    max_iter: int = 100
    init: str = "k-medoids++"
    seed: int = 0
    random_state: object = None  # None: the global generator, seeded with ``seed``
    rows: object = None  # () -> positions of the candidate rows, or None
    generic: bool = False
    _points: object = field(default=None, repr=False)
    _expected: object = field(default=None, repr=False)

    def points(self) -> np.ndarray:
        if self._points is None:
            self._points = self.make()
        return self._points

    def subset(self):
        return None if self.rows is None else self.rows()

    def candidates(self) -> np.ndarray:
        return self.points() if self.rows is None else self.points()[self.rows()]

    def expected(self):
        """The oracle's ``Result`` under the case's seed, computed once (warnings are the tests' business: silenced here)."""
        if self._expected is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                np.random.seed(self.seed)
                self._expected = oracle.k_medoids(self.candidates(), self.k, self.max_iter, self.init, self.random_state)
        return self._expected


def _normal(N, d, shift=0):
    return lambda: np.random.default_rng(1000 * N + d + shift).standard_normal((N, d))


GENERIC_SHAPES = [(63, 3), (64, 3), (65, 3), (255, 3), (256, 3), (257, 3), (1000, 20), (300, 33), (200, 70), (200, 97)] + \
                 [(130, d) for d in (2, 4, 5, 8, 9, 12, 13, 16, 17, 21, 24, 25, 32)]

# seeds of the global generator to be replaced should the oracle meet bit-equal ties under more than one case in ten
# (name -> shift; tests/test_pam_cpu.py::test_ties_are_rare_on_generic_points).  None so far: 2 of 69 cases meet one.
SEED_SHIFT: dict = {}


def generic_cases():
    out = []
    for N, d in GENERIC_SHAPES:
        for k in sorted({1, 2, min(12, N // 20)}):
            name = f"generic-{N}x{d}-k{k}"
            out.append(Case(name, _normal(N, d), k, seed=N + 7 * d + k + SEED_SHIFT.get(name, 0), generic=True))
    return out


def edge_cases():
    out = [Case(f"edge-{N}x{d}-k{k}", _normal(N, d), k, seed=N + k) for (N, d) in ((1, 1), (2, 1), (3, 2)) for k in range(1, N + 1)]
    out.append(Case("edge-65x3-k65", _normal(65, 3), 65, seed=1))
    out.append(Case("edge-65x3-k65-random", _normal(65, 3), 65, init="random", seed=2))
    out.append(Case("edge-40x400-k40", _normal(40, 400), 40, seed=3))  # 8-medoid LDS tiles: five of them
    out.append(Case("edge-60x200-k3", _normal(60, 200), 3, seed=5))  # 16-column LDS tiles
    out.append(Case("edge-30x768-k2", _normal(30, 768), 2, seed=6))  # the widest row
    out.append(Case("edge-300x3-k150-random", _normal(300, 3), 150, init="random", seed=4))  # many one- and two-member clusters
    return out


def grid_cases():
    out = []
    for name, (levels, spans) in fc.GRIDS.items():
        out.append(Case(f"grid-{name}-kpp", fc._grid(levels, spans), 10 if np.prod(levels) > 27 else 5, seed=11))
        out.append(Case(f"grid-{name}-random", fc._grid(levels, spans), 10 if np.prod(levels) > 27 else 5, init="random", seed=12))
    return out


def _duplicates():
    X = np.random.default_rng(77).standard_normal((40, 4))
    return np.vstack([X, X[5:35]])[np.random.default_rng(78).permutation(70)]


# a seed under which rs.choice(70, 6, replace=False) holds two identical rows of _duplicates() (found by search on the CPU;
# tests/test_pam_cpu.py checks that it still does)
DUPLICATE_DRAW_SEED = 9


def degenerate_cases():
    return [
        Case("duplicates-kpp", _duplicates, 6, seed=3),
        Case("duplicates-random", _duplicates, 6, init="random", seed=4),
        Case("duplicates-random-identical-draw", _duplicates, 6, init="random", seed=DUPLICATE_DRAW_SEED),
        Case("identical-rows", lambda: np.full((9, 3), 0.25), 3, seed=1),
    ]


def max_iter_cases():
    return [
        Case("max-iter-0", _normal(300, 5), 6, max_iter=0, seed=5),
        Case("max-iter-0-random", _normal(300, 5), 6, max_iter=0, init="random", seed=5),
        Case("max-iter-1-needs-more", _normal(300, 5), 6, max_iter=1, seed=5),
        Case("int-random-state", _normal(300, 5), 6, seed=99, random_state=1234),
    ]


def _half(N, seed):
    return lambda: np.flatnonzero(np.random.default_rng(seed).random(N) < 0.5)


def subset_cases():
    return [
        Case("subset-600x7-k8", _normal(600, 7), 8, seed=6, rows=_half(600, 1)),
        Case("subset-grid-6^3-k10", fc._grid([6] * 3), 10, seed=7, rows=_half(216, 2)),
    ]


def _outlier():
    X = np.random.default_rng(31).standard_normal((700, 3))
    X[333] = [60.0, -60.0, 60.0]
    return X


def outlier_cases():
    return [Case("outlier-700x3-k3", _outlier, 3, seed=8)]


def _long():
    return np.random.default_rng(16700).standard_normal((16700, 2))


LONG = Case("long-16700x2-k3", _long, 3, max_iter=2, seed=9)


def all_cases():
    """Every case small enough for the CPU oracle in a blink (the long one is kept apart)."""
    return generic_cases() + edge_cases() + grid_cases() + degenerate_cases() + max_iter_cases() + subset_cases() + outlier_cases()
