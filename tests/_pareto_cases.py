"""TEST INFRASTRUCTURE - the multi-target ``make_grid`` problems of ``tests/test_nehvi_gpu.py::_setup`` (n = 24, N = 150, d = 3; targets
from its ``_targets``), built once per (m, signs) and shared by ``tests/test_nparego_gpu.py`` and ``tests/test_qnehvi_gpu.py``: the
device's fitted engines and oracle models that carry the device fit's hyper-parameters."""

import numpy as np

from _problems import make_grid

_BUILT = {}


def targets(X, rng, noise=0.05):
    f1 = -((X - 0.25) ** 2).sum(1) + noise * rng.standard_normal(len(X))
    f2 = -((X - 0.75) ** 2).sum(1) + noise * rng.standard_normal(len(X))
    f3 = -np.abs(X - 0.5).sum(1) + noise * rng.standard_normal(len(X))
    return np.stack([f1, f2, f3], 1)


def setup(m, signs=None, n=24, N=150, d=3, seed=0):
    """(X [N, d], Xt [n, d], Y [n, m], signs [m], engines, oracle models); cached - callers leave all of it unchanged."""
    from baybe_amd import engine, gp_spec
    from oracle import gp_oracle as go

    signs = np.ones(m) if signs is None else np.asarray(signs, float)
    key = (m, tuple(signs), n, N, d, seed)
    if key not in _BUILT:
        rng = np.random.default_rng(seed)
        X = make_grid(N, d, seed)
        Xt = make_grid(4 * n, d, seed + 1)[:n]
        Y = targets(Xt, rng)[:, :m]
        engines, models = [], []
        for o in range(m):
            g = engine.HipGP(0)
            g.set_model(gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), Xt, Y[:, o])
            fi = g.fit()
            engines.append(g)
            models.append(go.fit_gp(go.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), Xt, Y[:, o],
                                    params=go.GPParams(fi.params.lengthscale, fi.params.noise, fi.params.mean)))
        _BUILT[key] = (X, Xt, Y, signs, engines, models)
    return _BUILT[key]


def coincides_with_baseline(X, Xt):
    """Candidates that coincide with a baseline row: their conditional variance is rounding noise around zero, and whether the 1e-8
    jitter applies depends on its sign (tests/test_nehvi_gpu.py::test_scores_match_oracle) - excluded from parity, held to
    "no improvement"."""
    return np.array([(np.abs(Xt - x).sum(1) < 1e-12).any() for x in X])
