"""Seeded models shared by tests/test_continuous_cpu.py and tests/test_continuous_gpu.py: two discrete numerical columns in front,
continuous columns behind them, scaling bounds that are not the unit box (the chain rule through the normalisation is part of
what is tested)."""

from __future__ import annotations

import numpy as np

from _problems import oracle_params, oracle_spec


def make_case(kernel: str, use_os: bool, n: int, d_cont: int, seed: int, noise: float = 0.02):
    """(spec, params, X_train, y, lo, hi) of a model over 2 discrete + ``d_cont`` continuous columns."""
    from baybe_amd import gp_spec

    rng = np.random.default_rng(seed)
    d = 2 + d_cont
    lo = rng.uniform(-2.0, 0.0, d)
    hi = lo + rng.uniform(0.5, 1.5, d)
    U = rng.random((n, d))
    U[:, :2] = rng.integers(0, 5, size=(n, 2)) / 4.0
    Xt = lo + U * (hi - lo)
    y = 3.0 - 2.0 * ((U - 0.4) ** 2).sum(axis=1) + 0.05 * rng.normal(size=n)
    spec = gp_spec.GPSpec.baybe_default(d, lo, hi, kernel=kernel)
    spec.use_outputscale = bool(use_os)
    ls = 0.15 * np.sqrt(d) * (0.7 + 0.6 * rng.random(d))  # ~0.4 of the box at d = 8: a step of 1e-4 is in the h^2 regime
    p = gp_spec.GPParams(ls, noise, 0.1, 1.7 if use_os else 1.0)
    return spec, p, Xt, y, lo, hi


def oracle_model(spec, p, Xt, y):
    from oracle import gp_oracle as go

    return go.GPModel(oracle_spec(spec), oracle_params(spec, p), Xt, y)


def random_rows(lo, hi, N: int, seed: int, spread: float = 1.0):
    """N rows of the box; ``spread`` < 1 keeps the continuous columns within that fraction of the box around its centre.  The
    finite-difference checks use 0.3: rows a fraction of a lengthscale apart have cross-covariances of the size of the kernel
    terms they are differences of, so that 16 eps |f| / h covers the rounding of the difference quotient of EVERY entry (a
    cross-covariance of far-apart rows is a small difference of large terms, and its quotient's rounding is set by the terms)."""
    rng = np.random.default_rng(seed)
    U = 0.5 + spread * (rng.random((N, len(lo))) - 0.5)
    U[:, :2] = rng.integers(0, 5, size=(N, 2)) / 4.0
    return lo + U * (hi - lo)
