"""Writes ``tests/golden/gmm_reference_selection.npz``: for the generic-position cases of ``tests/_gmm_cases.py`` the selection the
reference's ``GaussianMixtureClusteringRecommender`` really makes - ``_make_selection_default``
(``baybe/recommenders/pure/nonpredictive/clustering.py:55-76``: ``predict``, then one ``np.random.choice`` among the members of every
label of ``np.unique``) - from scikit-learn's own ``GaussianMixture(n_components=k, n_init=n_init).fit(P)``, with the global
``np.random`` generator seeded per case, and scikit-learn's ``lower_bound_``.  Per case name an int64 array (the selection) and, under
``<name>:lower_bound``, a float64 scalar.

Run where scikit-learn imports (``python tests/golden/make_gmm_golden.py``).  The inputs are regenerated from the cases' seeds.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))


def reference_selection(model, points) -> list:
    """What the reference's default selector does, in this project's words: for every label ``predict`` gives, ascending, one draw of
    the global generator among the positions that carry it."""
    labels = model.predict(points)
    picks = []
    for c in np.unique(labels):
        members = np.flatnonzero(labels == c)
        picks.append(int(np.random.choice(members)))
    return picks


def main():
    import _gmm_cases
    from sklearn.mixture import GaussianMixture

    out = {}
    for case in _gmm_cases.generic_cases():
        np.random.seed(case.seed)
        model = GaussianMixture(n_components=case.k, **case.kwargs()).fit(case.points())
        out[case.name] = np.asarray(reference_selection(model, case.points()), dtype=np.int64)
        out[case.name + ":lower_bound"] = np.float64(model.lower_bound_)
    np.savez_compressed(HERE / "gmm_reference_selection.npz", **out)
    print(f"{len(out) // 2} cases -> {HERE / 'gmm_reference_selection.npz'}")


if __name__ == "__main__":
    main()
