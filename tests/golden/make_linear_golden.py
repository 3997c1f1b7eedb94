"""Writes tests/golden/linear_golden.npz: the stored cases of tests/_linear_cases.py, each a fit by scikit-learn's ARDRegression (1.7.2
when the committed copy was made) on seeded synthetic data - the model arrays, the scaler constants, 257 candidate rows and
scikit-learn's OWN ``predict(return_std=True)`` on them, which is what the device pass is held to on machines without scikit-learn.
``tests/test_linear_cpu.py::test_golden_file_equals_a_fresh_fit`` keeps the file honest.

    python tests/golden/make_linear_golden.py
"""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import _linear_cases as lc  # noqa: E402


def build() -> dict:
    out = {}
    for name in lc.CASES:
        for key, value in lc.fit_case(name).items():
            out[f"{name}__{key}"] = value
    return out


if __name__ == "__main__":
    np.savez_compressed(lc.GOLDEN, **build())
    print(lc.GOLDEN, lc.GOLDEN.stat().st_size, "bytes")
