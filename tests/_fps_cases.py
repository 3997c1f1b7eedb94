"""TEST INFRASTRUCTURE - farthest-point-sampling cases shared by tests/test_fps_cpu.py and tests/test_fps_gpu.py.

A case is a ``Case``: seeded points, the call's arguments, the seed of the global ``np.random`` generator, optionally a mask of
live rows.  Inputs are regenerated from seeds, so the golden file (tests/golden/fps_reference_picks.npz) holds only picks.

* generic   seeded standard-normal points (no ties): held to the oracle AND to the reference's own picks.  Shapes: the edge sizes
            of the 64-row column tile and the 256-row row tile, d on both sides of every register-form width of the all-pairs
            kernel (2, 4, 8, 12, 16, 20, 24, 32) and two generic-form widths.
* planted   a cloud in the unit ball plus two points 20 apart, placed by RANK (the last column, the most significant sort key,
            ascends with the rank): inside one tile, in the first and the last row, both in the final partial tile, both masked
            out; N = 800 spans four row tiles and thirteen column tiles, the last of each partial.  One case beyond 64 row tiles,
            where a workgroup's segment of j grows to two row tiles.
* grids     product grids, standard-scaled: massive exact ties, held to the oracle's tie rule only.
* duplicates / identical / single point, and masks with about half the rows dead.
* edge      the widths of the all-pairs kernels that the generic shapes leave out, held to the oracle only.
"""

from __future__ import annotations

import itertools
from dataclasses import dataclass, field

import numpy as np

import _oracle_fps as oracle


@dataclass
class Case:
    name: str
    make: object  # () -> points [N, d]
    n_samples: int
    initialization: object = "farthest"
    random_tie_break: bool = False
    seed: int = 0
    alive: object = None  # () -> bool [N] or None
    generic: bool = False
    _points: object = field(default=None, repr=False)

    def points(self) -> np.ndarray:
        if self._points is None:
            self._points = self.make()
        return self._points

    def mask(self):
        return None if self.alive is None else self.alive()

    def expected(self):
        """(indices, d2) of the oracle under the case's seed (warnings pass through)."""
        np.random.seed(self.seed)
        return oracle.farthest_point_sampling(self.points(), self.n_samples, self.initialization, self.random_tie_break, self.mask())


GENERIC_SHAPES = [(2, 1), (3, 2), (63, 3), (64, 3), (65, 3), (257, 3), (1000, 20), (300, 33), (200, 70),
                  (130, 10), (130, 15), (130, 22), (130, 30)]


# The reference's distance matrix (sklearn's |x|^2 + |y|^2 - 2 x.y form) is not symmetric to the last bit: about one entry in ten
# differs from its mirror image by an ulp.  d(a, b) and d(b, a) are mathematically tied, so where the two entries of the LARGEST
# distance differ the wrong way round, the reference's row-major argmax lands on (b, a) and its "farthest" start comes out as
# [b, a] instead of [a, b] - the same pair, resolved by rounding like the ties on grids.  The seed 1000 N + d of the 65 x 3 shape is
# such an input (tests/test_fps_cpu.py keeps it as a documented case); its generic case uses the next seed.
SEED_SHIFT = {(65, 3): 1}
MIRRORED_START = (65, 3)


def _normal(N, d, shift=None):
    shift = SEED_SHIFT.get((N, d), 0) if shift is None else shift
    return lambda: np.random.default_rng(1000 * N + d + shift).standard_normal((N, d))


def generic_cases():
    out = []
    for N, d in GENERIC_SHAPES:
        sizes = sorted({1, 2, min(12, N)} | ({N} if N <= 65 else set()))
        inits = [("farthest", "farthest"), ("random", "random"), ("index", [N - 1, 0, N // 2] if N >= 3 else [N - 1, 0])]
        for (iname, init), rtb, ns in itertools.product(inits, (False, True), sizes):
            out.append(Case(f"generic-{N}x{d}-{iname}-{'rtb' if rtb else 'det'}-n{ns}", _normal(N, d), ns, init, rtb,
                            seed=N + 7 * d + ns, generic=True))
    return out


def _planted(N, d, ra, rb, seed):
    """Unit-ball cloud + two planted points at distance 20, at ranks ra < rb; rows shuffled."""

    def make():
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((N, d))
        X *= (rng.random(N) ** (1.0 / d) / np.linalg.norm(X, axis=1))[:, None]  # uniform in the unit ball
        u = np.zeros(d)
        u[0] = 10.0
        X[ra], X[rb] = u, -u
        X[:, -1] = np.arange(N) / N  # the most significant sort key ascends with the row: row r has rank r
        return X[rng.permutation(N)]

    return make


def _planted_mask(N, d, seed):
    """Live rows of a planted case without the two planted points (the rows whose first coordinate is +-10)."""
    return lambda: np.abs(_planted(N, d, 0, N - 1, seed)()[:, 0]) < 5.0


def planted_cases():
    N, d = 800, 3
    out = [
        Case("planted-one-tile", _planted(N, d, 399, 400, 1), 6),
        Case("planted-first-last", _planted(N, d, 0, N - 1, 2), 6),
        Case("planted-final-partial-tile", _planted(N, d, 770, 790, 3), 6),
        Case("planted-final-partial-tile-random-ties", _planted(N, d, 770, 790, 3), 6, "farthest", True, seed=5),
        Case("planted-masked-out", _planted(N, d, 0, N - 1, 4), 6, alive=_planted_mask(N, d, 4)),
        Case("planted-two-tile-segments", _planted(16700, 2, 5, 16650, 5), 3),
    ]
    return out


def _grid(levels, spans=None):
    def make():
        axes = [np.linspace(0.0, 1.0 if spans is None else spans[i], n) for i, n in enumerate(levels)]
        X = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(levels))
        return oracle.standard_scale(X)

    return make


GRIDS = {"3^3": ([3] * 3, None), "4^4": ([4] * 4, None), "2^6": ([2] * 6, None), "6^3": ([6] * 3, None),
         "2x2x3x5x4": ([2, 2, 3, 5, 4], [1.0, 3.0, 0.5, 7.0, 2.0])}


def grid_cases():
    out = []
    for name, (levels, spans) in GRIDS.items():
        for init, rtb in (("farthest", False), ("farthest", True), ("random", True), ("random", False)):
            out.append(Case(f"grid-{name}-{init}-{'rtb' if rtb else 'det'}", _grid(levels, spans), 10, init, rtb, seed=11))
    return out


def _duplicates():
    X = np.random.default_rng(77).standard_normal((40, 4))
    return np.vstack([X, X[5:15]])[np.random.default_rng(78).permutation(50)]


def degenerate_cases():
    return [
        Case("duplicates-det", _duplicates, 45),
        Case("duplicates-rtb", _duplicates, 45, "farthest", True, seed=3),
        Case("duplicates-random-start", _duplicates, 45, "random", True, seed=4),
        Case("identical", lambda: np.full((9, 3), 0.25), 4),
        Case("single-point", lambda: np.array([[1.0, 2.0]]), 1),
    ]


def _half(N, seed):
    return lambda: np.random.default_rng(seed).random(N) < 0.5


def mask_cases():
    return [
        Case("mask-257x3-det", _normal(257, 3), 12, alive=_half(257, 1)),
        Case("mask-257x3-random", _normal(257, 3), 12, "random", True, seed=9, alive=_half(257, 2)),
        Case("mask-1000x20-rtb", _normal(1000, 20), 12, "farthest", True, seed=10, alive=_half(1000, 3)),
        Case("mask-300x33-det", _normal(300, 33), 12, alive=_half(300, 4)),
        Case("mask-grid-6^3-det", _grid([6] * 3), 10, alive=_half(216, 5)),
        Case("mask-grid-6^3-rtb", _grid([6] * 3), 10, "farthest", True, seed=12, alive=_half(216, 6)),
    ]


# Every instantiation of the all-pairs walk that the shapes above leave out: d at the upper edge of a register-form width and one
# past it (so the next width runs with its padding columns), the register form of width 8, and the generic form's 32-, 16- and
# 8-row tiles (d = 97, 200, 400 and the limit 768).  Held to the oracle only (generic=False: no entry in the golden file).  On
# these seeds the oracle meets no bit-equal tie, neither in the farthest pair nor in a pick (the largest d2 over all pairs and the
# largest minimum d2 of every pick each occur once), so no seed needed a shift.
EDGE_SHAPES = [(130, d) for d in (4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)] + [(70, 97), (70, 200), (40, 400), (30, 768)]
EDGE_MASKED = [(130, 8), (70, 200)]


def edge_cases():
    out = [Case(f"edge-{N}x{d}-farthest-det-n3", _normal(N, d), 3) for N, d in EDGE_SHAPES]
    out += [Case(f"edge-mask-{N}x{d}-farthest-det-n3", _normal(N, d), 3, alive=_half(N, 20 + d)) for N, d in EDGE_MASKED]
    return out


def all_cases():
    return generic_cases() + planted_cases() + grid_cases() + degenerate_cases() + mask_cases() + edge_cases()
