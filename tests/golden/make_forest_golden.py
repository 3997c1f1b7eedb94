"""Writes tests/golden/forest_cases.npz: the small forest fixtures of tests/_forest_cases.py, fitted with scikit-learn (1.7.2 when the
committed copy was made) under their fixed random_state - per case the packed node arrays, the candidate rows, the training rows and
scikit-learn's OWN ``estimator.predict`` outputs for both row sets, which is what the device traversal is held to bit for bit on
machines without scikit-learn.  ``tests/test_forest_cpu.py::test_golden_file_equals_a_fresh_fit`` keeps the file honest.
Writes tests/golden/forest_mixed.npz as well: the same arrays for ``MIXED``, the forest with trees of 199 to 1399 nodes
(``tests/test_forest_cpu.py::test_mixed_file_equals_a_fresh_fit``).

    python tests/golden/make_forest_golden.py
"""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import _forest_cases as fc  # noqa: E402
from baybe_amd.forest import pack_forest  # noqa: E402


def build() -> dict:
    out = {}
    for name in fc.CASES:
        if "like" in fc.CASES[name]:
            continue
        estimators, X, train_x, _ = fc.fit_case(name)
        packed = pack_forest(estimators)
        for k in fc.PACKED_KEYS:
            out[f"{name}__{k}"] = packed[k]
        out[f"{name}__X"], out[f"{name}__train_x"] = X, train_x
        out[f"{name}__pred"] = np.stack([e.predict(X) for e in estimators])
        out[f"{name}__pred_train"] = np.stack([e.predict(train_x) for e in estimators])
    return out


def build_mixed() -> dict:
    estimators, X, train_x, _ = fc.fit_mixed()
    out = dict(pack_forest(estimators))
    out["X"], out["train_x"] = X, train_x
    out["pred"] = np.stack([e.predict(X) for e in estimators])
    out["pred_train"] = np.stack([e.predict(train_x) for e in estimators])
    return out


if __name__ == "__main__":
    np.savez_compressed(fc.GOLDEN, **build())
    print(fc.GOLDEN, fc.GOLDEN.stat().st_size, "bytes")
    np.savez_compressed(fc.MIXED_GOLDEN, **build_mixed())
    print(fc.MIXED_GOLDEN, fc.MIXED_GOLDEN.stat().st_size, "bytes")
