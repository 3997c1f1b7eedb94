"""Writes ``tests/golden/pam_reference_medoids.npz``: the REFERENCE's own ``KMedoids(n_clusters=k, max_iter=100,
init="k-medoids++").fit(P).medoid_indices_`` (``baybe/utils/clustering_algorithms/third_party/kmedoids.py``, sklearn's
``pairwise_distances`` underneath; the parameters are ``PAMClusteringRecommender``'s defaults) for the generic-position cases of
``tests/_pam_cases.py``, one int64 array per case name, with the global ``np.random`` generator seeded per case.

Run where the reference tree imports (``python tests/golden/make_pam_golden.py``).  Only index arrays are stored: the inputs are
regenerated from the cases' seeds.  Grids, duplicate rows and small clusters are not recorded - there the reference's choice among
mathematically tied costs follows the rounding of its GEMM-form distances, which is not a contract.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))


def main():
    import _pam_cases
    from _reference import reference_baybe

    reference_baybe()
    from baybe.utils.clustering_algorithms import KMedoids

    medoids = {}
    for case in _pam_cases.generic_cases():
        np.random.seed(case.seed)
        model = KMedoids(n_clusters=case.k, max_iter=100, init="k-medoids++").fit(case.points())
        medoids[case.name] = np.asarray(model.medoid_indices_, dtype=np.int64)
    np.savez_compressed(HERE / "pam_reference_medoids.npz", **medoids)
    print(f"{len(medoids)} cases -> {HERE / 'pam_reference_medoids.npz'}")


if __name__ == "__main__":
    main()
