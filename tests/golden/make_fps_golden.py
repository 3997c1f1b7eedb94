"""Writes ``tests/golden/fps_reference_picks.npz``: the REFERENCE's own ``farthest_point_sampling`` picks
(``baybe/utils/sampling_algorithms.py:15-172``, sklearn's ``pairwise_distances`` underneath) for the generic-position cases of
``tests/_fps_cases.py``, one int64 array per case name, with the global ``np.random`` generator seeded per case.

Run where the reference tree imports (``python tests/golden/make_fps_golden.py``).  Only picks are stored: the inputs are
regenerated from the cases' seeds.  Grids and duplicate rows are not recorded - there the reference's choice among mathematically
tied points follows the rounding of its GEMM-form distances, which is not a contract.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))


def main():
    import _fps_cases
    from _reference import reference_baybe

    reference_baybe()
    from baybe.utils.sampling_algorithms import farthest_point_sampling

    picks = {}
    for case in _fps_cases.generic_cases():
        np.random.seed(case.seed)
        got = farthest_point_sampling(case.points(), case.n_samples, case.initialization, case.random_tie_break)
        picks[case.name] = np.asarray([int(i) for i in got], dtype=np.int64)
    np.savez_compressed(HERE / "fps_reference_picks.npz", **picks)
    print(f"{len(picks)} cases -> {HERE / 'fps_reference_picks.npz'}")


if __name__ == "__main__":
    main()
