"""TEST INFRASTRUCTURE - k-means cases shared by tests/test_kmeans_cpu.py and tests/test_kmeans_gpu.py.

A case is a ``Case`` as in ``_pam_cases``: seeded points, the call's arguments, the seed of the global ``np.random`` generator (or
an int ``random_state``), optionally the candidate rows.  Inputs are regenerated from seeds, so the golden file
(tests/golden/kmeans_reference_selection.npz) holds only the reference's selections.

* generic   seeded standard-normal points, held to the oracle AND to scikit-learn.  Every one must clear the oracle's margin
            conditions (``Result.clears()``): a case that does not gets another seed (``SEED_SHIFT``), never a looser test.  Shapes:
            the edges of the 256-position tile, 1000 x 20 with the reference's 50 restarts (three restart tiles), wide rows, and
            130 x d on both sides of d = 16, up to which the pass kernel keeps the tile's coordinates in LDS.
* edge      1, 2, 3 rows with every k; k = N at 65 rows; d = 768; k * d beyond what LDS holds for one restart (k = 11 at d = 768:
            the one-restart form with the centres streamed in chunks) at N = k = 11, the smallest N there is, and at 40 rows;
            50 restarts of a small k * d (48 restarts share a tile: two tiles).
* exact     integer-valued points: a product grid and duplicated rows.  Bit-equal ties everywhere, and one seed for which
            ``init="random"`` draws two identical rows, so that a cluster is empty and relocated.  Sums of integers are exact in any
            order, so the centres - and with them every tie - are the same bits on the device as in the oracle: held to the
            oracle's result wherever its non-zero margins clear the conditions (``Result.decidable()``).
* grids     product grids from ``_fps_cases.GRIDS`` and ``_pam_cases._duplicates``, standard-scaled floats: mathematically tied
            distances that differ in the last bits.  No decision-by-decision comparison is possible; the result must be a valid
            clustering (tests/test_kmeans_gpu.py::_check_valid).
* others    max_iter 0 (through ``_kmeans_fit``: the public calls refuse it as scikit-learn does) and 1, init="random", an int
            ``random_state``, a candidate subset of a larger resident matrix.
* long      16 700 x 2, k = 3, n_init = 2, max_iter = 2: some 66 position tiles (GPU test only).
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np

import _fps_cases as fc
import _oracle_kmeans as oracle
import _pam_cases as pc


@dataclass
class Case(pc.Case):
    n_init: object = 3
    max_iter: int = 300
    tol: float = 1e-4
    init: str = "k-means++"
    exact: bool = False  # integer-valued points: sums are exact, ties are the same bits everywhere

    def kwargs(self) -> dict:
        return dict(n_init=self.n_init, max_iter=self.max_iter, tol=self.tol, init=self.init)

    def expected(self):
        """The oracle's ``Result`` under the case's seed, computed once."""
        if self._expected is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                np.random.seed(self.seed)
                self._expected = oracle.k_means(self.candidates(), self.k, random_state_=self.random_state, **self.kwargs())
        return self._expected


_normal = pc._normal

X_LDS_MAX_D = 16  # the pass kernel keeps the tile's coordinates in LDS up to this width (KM_X_LDS_MAX_D)
GENERIC_SHAPES = [(63, 3), (64, 3), (65, 3), (255, 3), (256, 3), (257, 3), (1000, 20), (300, 33), (200, 70)] + \
                 [(130, d) for d in (2, X_LDS_MAX_D - 1, X_LDS_MAX_D, X_LDS_MAX_D + 1)]

# seeds of the global generator replaced because the oracle's margins did not clear the conditions (name -> shift)
SEED_SHIFT: dict = {}


def generic_cases():
    out = []
    for N, d in GENERIC_SHAPES:
        for k in sorted({1, 2, min(12, N // 20)}):
            name = f"generic-{N}x{d}-k{k}"
            out.append(Case(name, _normal(N, d), k, seed=N + 7 * d + k + SEED_SHIFT.get(name, 0), generic=True,
                            n_init=50 if (N, d) == (1000, 20) else 3, max_iter=1000))
    return out


def edge_cases():
    out = [Case(f"edge-{N}x{d}-k{k}", _normal(N, d), k, seed=N + k) for (N, d) in ((1, 1), (2, 1), (3, 2)) for k in range(1, N + 1)]
    out.append(Case("edge-65x3-k65", _normal(65, 3), 65, seed=1))
    out.append(Case("edge-30x768-k2", _normal(30, 768), 2, seed=6))
    out.append(Case("edge-fallback-11x768-k11", _normal(11, 768), 11, seed=7))
    out.append(Case("edge-fallback-40x768-k11", _normal(40, 768), 11, seed=8))
    out.append(Case("edge-two-restart-tiles-130x3-k3", _normal(130, 3), 3, seed=9, n_init=50))
    return out


def _int_grid():
    return np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3)


def _int_duplicates():
    X = np.random.default_rng(77).integers(-8, 9, (40, 4)).astype(np.float64)
    return np.vstack([X, X[5:35]])[np.random.default_rng(78).permutation(70)]


# a seed under which the first rs.choice(70, 6, replace=False) holds two identical rows of _int_duplicates() (found by search on the
# CPU; tests/test_kmeans_cpu.py checks that it still does)
DUPLICATE_DRAW_SEED = 9


def exact_cases():
    return [
        Case("exact-grid-5^3-k5", _int_grid, 5, seed=11, exact=True),
        Case("exact-grid-5^3-k5-random", _int_grid, 5, seed=12, init="random", exact=True),
        Case("exact-duplicates-k6", _int_duplicates, 6, seed=3, exact=True),
        Case("exact-duplicates-random-identical-draw", _int_duplicates, 6, seed=DUPLICATE_DRAW_SEED, init="random", n_init=1, exact=True),
        Case("exact-identical-rows", lambda: np.full((9, 3), 0.25), 3, seed=1, exact=True),
    ]


def grid_cases():
    out = []
    for name, (levels, spans) in fc.GRIDS.items():
        make = (lambda lv=levels, sp=spans: oracle.standard_scale(fc._grid(lv, sp)()))
        out.append(Case(f"grid-{name}-kpp", make, 10 if np.prod(levels) > 27 else 5, seed=11))
    out.append(Case("duplicates-kpp", pc._duplicates, 6, seed=3))
    return out


def other_cases():
    return [
        Case("max-iter-0", _normal(300, 5), 6, max_iter=0, seed=5),
        Case("max-iter-1", _normal(300, 5), 6, max_iter=1, seed=5),
        Case("init-random", _normal(300, 5), 6, init="random", seed=5),
        Case("init-random-auto", _normal(300, 5), 6, init="random", n_init="auto", seed=6),
        Case("n-init-auto", _normal(300, 5), 6, n_init="auto", seed=7),
        Case("int-random-state", _normal(300, 5), 6, seed=99, random_state=1234),
        Case("subset-600x7-k8", _normal(600, 7), 8, seed=6, rows=pc._half(600, 1)),
    ]


LONG = Case("long-16700x2-k3", pc._long, 3, n_init=2, max_iter=2, seed=9)


def all_cases():
    """Every case small enough for the CPU oracle (the long one is kept apart)."""
    return generic_cases() + edge_cases() + exact_cases() + grid_cases() + other_cases()
