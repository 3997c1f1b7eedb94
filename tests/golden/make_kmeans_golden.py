"""Writes ``tests/golden/kmeans_reference_selection.npz``: for the generic-position cases of ``tests/_kmeans_cases.py`` the selection
the reference's ``KMeansClusteringRecommender._make_selection_custom`` makes (``baybe/recommenders/pure/nonpredictive/clustering.py:
241-252``: ``pairwise_distances`` to the centres, ``predict``, other clusters' members set to infinity, ``argmin`` per column) from
scikit-learn's own ``KMeans(n_clusters=k, max_iter=1000, n_init=n_init).fit(P)``, one int64 array per case name, with the global
``np.random`` generator seeded per case.

Run where scikit-learn imports (``python tests/golden/make_kmeans_golden.py``).  Only index arrays are stored: the inputs are
regenerated from the cases' seeds.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))


def reference_selection(model, points) -> list:
    """The reference's own lines, restated."""
    from sklearn.metrics import pairwise_distances

    distances = pairwise_distances(points, model.cluster_centers_)
    predicted_clusters = model.predict(points)
    for k_cluster in range(model.cluster_centers_.shape[0]):
        distances[predicted_clusters != k_cluster, k_cluster] = np.inf
    return np.argmin(distances, axis=0).tolist()


def main():
    import _kmeans_cases
    from sklearn.cluster import KMeans

    out = {}
    for case in _kmeans_cases.generic_cases():
        np.random.seed(case.seed)
        model = KMeans(n_clusters=case.k, max_iter=case.max_iter, n_init=case.n_init).fit(case.points())
        out[case.name] = np.asarray(reference_selection(model, case.points()), dtype=np.int64)
    np.savez_compressed(HERE / "kmeans_reference_selection.npz", **out)
    print(f"{len(out)} cases -> {HERE / 'kmeans_reference_selection.npz'}")


if __name__ == "__main__":
    main()
