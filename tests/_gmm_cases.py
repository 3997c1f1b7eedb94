"""TEST INFRASTRUCTURE - Gaussian mixture cases shared by tests/test_gmm_cpu.py and tests/test_gmm_gpu.py.

A case is a ``Case`` as in ``_kmeans_cases``: seeded points, the call's arguments, the seed of the global ``np.random`` generator (or
an int ``random_state``), optionally the candidate rows.  Inputs are regenerated from seeds, so the golden file
(tests/golden/gmm_reference_selection.npz) holds only scikit-learn's selections and lower bounds.

* generic   seeded standard-normal points, held to the oracle AND to scikit-learn.  Every one must clear the oracle's conditions
            (``Result.clears()``: label gap >= 1e-6, stop gap >= 1e-6, restart gap >= 1e-9, condition number <= 1e4, no flagged
            restart): a case that does not gets another seed (``SEED_SHIFT``), never a looser test.  Shapes: the edges of the
            256-position tile, d on both sides of the 16-column MFMA block, two, three and four blocks, k in {1, 2, min(12, N // (4 d))}.
* edge      N = 2 with k = 1 and 2; k = N at 65 x 3 (every component a singleton: Sigma = reg_covar I); d = 1; d = 64 at 40 rows with
            k = 2 (fewer members than columns: reg_covar carries the factor); reg_covar = 0 with singletons (the flagged error, a
            returned flag); k = 100 at 300 x 3 (component chunks of the E-step).
* others    max_iter 0 and 1 (1 warns), init_params "k-means++" and "random_from_data", an int ``random_state``, a candidate subset
            of a larger resident matrix, duplicated rows.
* long      16 700 x 2, k = 3, max_iter = 2: some 66 position tiles, several strips (GPU test only).

``Case.tolerances()`` is the yardstick of the whole-fit comparison on the device: per quantity ``max(100 * |oracle(order="numpy") -
oracle(order="tiles")|, 1e-12)``, computed on the CPU.
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

import _oracle_gmm as oracle
import _pam_cases as pc


@dataclass
class Case(pc.Case):
    tol: float = 1e-3
    reg_covar: float = 1e-6
    max_iter: int = 100
    n_init: int = 1
    init_params: str = "kmeans"
    raises: bool = False  # the fit is the flagged error
    _tiles: object = field(default=None, repr=False)

    def kwargs(self) -> dict:
        return dict(tol=self.tol, reg_covar=self.reg_covar, max_iter=self.max_iter, n_init=self.n_init, init_params=self.init_params)

    def _run(self, order):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.random.seed(self.seed)
            try:
                return oracle.gaussian_mixture(self.candidates(), self.k, random_state_=self.random_state, order=order, **self.kwargs())
            except ValueError as err:
                return err

    def expected(self):
        """The oracle's ``Result`` under the case's seed (the ``ValueError`` for a flagged fit), computed once."""
        if self._expected is None:
            self._expected = self._run("numpy")
        return self._expected

    def tolerances(self) -> dict:
        """Per quantity ``max(100 * |numpy order - tile order|, 1e-12)``; ``same``: both orders took the same decisions."""
        if self._tiles is None:
            a, b = self.expected(), self._run("tiles")
            with np.errstate(invalid="ignore"):  # (max_iter = 0: both lower bounds are -inf)
                dev = {name: float(np.nan_to_num(np.max(np.abs(np.asarray(getattr(a, name)) - np.asarray(getattr(b, name))))))
                       for name in ("weights", "means", "covariances", "lower_bound")}
            self._tiles = {name: max(100 * v, 1e-12) for name, v in dev.items()}
            self._tiles["deviation"] = dev
            self._tiles["same"] = (a.n_iter == b.n_iter and a.best == b.best and a.labels.tolist() == b.labels.tolist())
        return self._tiles


_normal = pc._normal

GENERIC_SHAPES = [(63, 3), (255, 3), (256, 3), (257, 3), (130, 15), (130, 16), (130, 17), (1000, 20), (300, 33), (400, 64)]
THREE_RESTARTS = (257, 3)  # (with k > 1: the restarts of k = 1 are one and the same fit, a restart gap of 0 under every seed)

# seeds of the global generator replaced because the oracle's margins did not clear the conditions (name -> shift)
SEED_SHIFT: dict = {}


def generic_cases():
    out = []
    for N, d in GENERIC_SHAPES:
        for k in sorted({1, 2} | ({min(12, N // (4 * d))} if min(12, N // (4 * d)) >= 2 else set())):
            name = f"generic-{N}x{d}-k{k}"
            out.append(Case(name, _normal(N, d), k, seed=N + 7 * d + k + SEED_SHIFT.get(name, 0), generic=True,
                            n_init=3 if (N, d) == THREE_RESTARTS and k > 1 else 1))
    return out


def edge_cases():
    return [
        Case("edge-2x2-k1", _normal(2, 2), 1, seed=3),
        Case("edge-2x2-k2", _normal(2, 2), 2, seed=4),
        Case("edge-65x3-k65", _normal(65, 3), 65, seed=1),
        Case("edge-100x1-k3", _normal(100, 1), 3, seed=2),
        Case("edge-40x64-k2", _normal(40, 64), 2, seed=6),
        Case("edge-reg0-singletons-65x3-k65", _normal(65, 3), 65, seed=1, reg_covar=0.0, raises=True),
        Case("edge-300x3-k100", _normal(300, 3), 100, seed=5),
    ]


def other_cases():
    return [
        Case("max-iter-0", _normal(300, 5), 6, max_iter=0, seed=5),
        Case("max-iter-1", _normal(300, 5), 6, max_iter=1, seed=5),
        Case("init-kmeans++", _normal(300, 5), 4, init_params="k-means++", seed=5),
        Case("init-random-from-data", _normal(300, 5), 4, init_params="random_from_data", seed=6, n_init=2),
        Case("int-random-state", _normal(300, 5), 6, seed=99, random_state=1234),
        Case("subset-600x7-k8", _normal(600, 7), 8, seed=6, rows=pc._half(600, 1)),
        Case("duplicates", pc._duplicates, 6, seed=3),
    ]


LONG = Case("long-16700x2-k3", pc._long, 3, max_iter=2, seed=9)


def all_cases():
    """Every case small enough for the CPU oracle (the long one is kept apart)."""
    return generic_cases() + edge_cases() + other_cases()
