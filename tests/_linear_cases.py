"""Fixtures of the Bayesian linear (ARD) surrogate tests.

Stored cases (``tests/golden/linear_golden.npz``, written by ``tests/golden/make_linear_golden.py``): each is a fit by the installed
scikit-learn (1.7.2 when the committed copy was made) on seeded synthetic data - inputs drawn on a grid of 64ths inside per-column
scaling bounds, ``active`` non-zero true weights, Gaussian noise - and holds the model arrays, the scaler constants, 257 candidate rows
(one past a 256-row tile) and scikit-learn's OWN ``predict(return_std=True)`` on them (on the scaled inputs, in standardised units).

Synthetic packs (``synthetic_model``): a random symmetric PSD ``sigma_`` of half rank, nudged off symmetry by 1e-11 as the Woodbury branch
leaves it, with d = k + 8 columns of which k are kept - for the edges k = 0, 1, 16, 17, 32, 33, 48 and 512.

The end-to-end grid (``grid_context``): 216 rows, 18 noisy measurements of a near-linear response.
"""

from pathlib import Path
from types import SimpleNamespace

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "linear_golden.npz"
MODEL_KEYS = ("lambda_", "threshold_lambda", "coef_", "intercept_", "sigma_", "alpha_")
N_CAND = 257
ANALYTIC_KINDS = ("PM", "PSTD", "UCB", "EI", "LogEI", "PI")
MC_KINDS = ("qLogEI", "qEI", "qPI", "qSR", "qUCB", "qPSTD")
PICK_KINDS = ("qLogEI", "EI", "UCB")  # the acquisition functions of the end-to-end picks
PICK_MARGIN = 1e-6
SYNTHETIC_K = (0, 1, 16, 17, 32, 33, 48, 512)

# name -> training rows n, columns d, non-zero true weights, noise deviation, seed; `kept` is what scikit-learn 1.7.2 keeps
CASES = {
    "n40_d6": dict(n=40, d=6, active=6, noise=0.1, seed=1, kept=6, woodbury=False),
    "n60_d20": dict(n=60, d=20, active=6, noise=0.1, seed=6, kept=8, woodbury=False),
    "n12_d30": dict(n=12, d=30, active=2, noise=0.05, seed=12, kept=7, woodbury=True),
    "n100_d70": dict(n=100, d=70, active=58, noise=0.1, seed=19, kept=58, woodbury=False),
    "n30_d130": dict(n=30, d=130, active=25, noise=0.05, seed=3, kept=25, woodbury=True),
    "n200_d300": dict(n=200, d=300, active=161, noise=0.1, seed=2, kept=161, woodbury=True),
}


def case_data(name: str):
    """(train_x [n, d], train_y [n], lo [d], hi [d], candidates [257, d]) of a stored case - raw rows, inside [lo, hi]."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    n, d = c["n"], c["d"]
    lo = rng.integers(-4, 5, d).astype(np.float64)
    hi = lo + rng.integers(1, 5, d).astype(np.float64)
    U = rng.integers(0, 65, (n, d)) / 64.0
    w = np.zeros(d)
    w[rng.permutation(d)[: c["active"]]] = rng.choice([-1.0, 1.0], c["active"]) * (0.5 + rng.random(c["active"]))
    y = 3.0 + 2.0 * (U @ w + c["noise"] * rng.standard_normal(n))
    C = rng.integers(0, 65, (N_CAND, d)) / 64.0
    return lo + (hi - lo) * U, y, lo, hi, lo + (hi - lo) * C


def fit_case(name: str) -> dict:
    """The arrays of a stored case, fitted afresh with scikit-learn the way the surrogate fits."""
    from sklearn.linear_model import ARDRegression

    from baybe_amd.linear import scale_inputs, standardize_targets

    train_x, train_y, lo, hi, X = case_data(name)
    y_std, ybar, s = standardize_targets(train_y)
    model = ARDRegression().fit(scale_inputs(train_x, lo, hi), y_std)
    mean, std = model.predict(scale_inputs(X, lo, hi), return_std=True)
    out = {k: np.asarray(getattr(model, k), dtype=np.float64) for k in MODEL_KEYS}
    out.update(lo=lo, hi=hi, ybar=np.float64(ybar), s=np.float64(s), X=X, pred_mean=mean, pred_std=std, n_iter=np.int64(model.n_iter_))
    return out


def as_model(g: dict) -> SimpleNamespace:
    """What ``pack_linear`` reads of a fitted ``ARDRegression``, from stored arrays."""
    return SimpleNamespace(lambda_=g["lambda_"], threshold_lambda=float(g["threshold_lambda"]), coef_=g["coef_"],
                           intercept_=float(g["intercept_"]), sigma_=g["sigma_"], alpha_=float(g["alpha_"]))


def load_golden() -> dict:
    """name -> the arrays ``fit_case`` returns, from the committed file."""
    out = {}
    with np.load(GOLDEN) as z:
        for name in CASES:
            out[name] = {key.split("__", 1)[1]: z[key] for key in z.files if key.startswith(name + "__")}
    return out


def synthetic_model(k: int, seed: int = 0) -> dict:
    """A model that scikit-learn did not fit: d = k + 8 columns, k of them kept, ``sigma_`` symmetric PSD of rank ceil(k / 2) plus an
    antisymmetric part of 1e-11; with the scaler constants, the un-standardisation and 257 candidate rows.  Same keys as a stored case
    (without scikit-learn's prediction)."""
    rng = np.random.default_rng(1000 + 17 * k + seed)
    d = k + 8
    kept = np.sort(rng.permutation(d)[:k])
    lam = np.full(d, 1e6)
    lam[kept] = 0.5 + rng.random(k)
    coef = np.zeros(d)
    coef[kept] = rng.standard_normal(k)
    A = rng.standard_normal((k, max(1, (k + 1) // 2)))
    sigma = A @ A.T / max(k, 1)
    skew = rng.standard_normal((k, k)) * 1e-11
    sigma = sigma + (skew - skew.T)
    lo = rng.integers(-4, 5, d).astype(np.float64)
    hi = lo + rng.integers(1, 5, d).astype(np.float64)
    X = lo + (hi - lo) * rng.random((N_CAND, d))
    return dict(lambda_=lam, threshold_lambda=np.float64(1e4), coef_=coef, intercept_=np.float64(0.375), sigma_=sigma,
                alpha_=np.float64(7.0), lo=lo, hi=hi, ybar=np.float64(-1.5), s=np.float64(2.5), X=X)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
GRID_SEED = 8


def grid_context(minimize: bool, transformation=None):
    """(search space, objective, measurements) of the end-to-end tests: a 6 x 6 x 6 grid with unequal scaling bounds, 18 measurements."""
    from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, SearchSpace, SingleTargetObjective

    vals = [np.arange(6) / 5.0, 2.0 + np.arange(6), -1.0 + 0.5 * np.arange(6)]
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", v) for i, v in enumerate(vals)])
    rng = np.random.default_rng(GRID_SEED)
    rows = rng.choice(len(space.discrete.exp_rep), 18, replace=False)
    meas = space.discrete.exp_rep.iloc[rows].reset_index(drop=True)
    x = meas.to_numpy()
    meas["y"] = 1.0 + 2.0 * x[:, 0] - 0.3 * x[:, 1] + 0.8 * x[:, 2] + 0.2 * rng.standard_normal(len(x))
    target = NumericalTarget("y", minimize=minimize)
    if transformation is not None:
        target.transformation = transformation
    return space, SingleTargetObjective(target), meas


GRID_TORCH_SEED = 1  # torch.manual_seed before a recommend() of the end-to-end tests
N_MC = 512  # the default n_mc_samples of the MC acquisition functions
BETA = 0.2  # ... and the default beta of UCB / qUCB


def grid_sampler_seed() -> int:
    """The MC sampler seed a recommend() draws after ``torch.manual_seed(GRID_TORCH_SEED)`` (the global generator is left alone)."""
    import torch

    from baybe_amd.engine import draw_sampler_seed

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(GRID_TORCH_SEED)
        return draw_sampler_seed()


def grid_oracle_moments(minimize: bool):
    """(mean [216], var [216], best_f) of the grid under the reference's path with scikit-learn itself (``_oracle_linear.fit_reference``)."""
    import _oracle_linear as ol

    space, obj, meas = grid_context(minimize)
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    train_x = space.transform(meas).to_numpy(dtype=np.float64)
    bounds = space.scaling_bounds.to_numpy(dtype=np.float64)
    mean, var, mean_train = ol.fit_reference(train_x, meas["y"].to_numpy(), bounds[0], bounds[1], comp)
    sign = -1.0 if minimize else 1.0
    return mean, var, float((sign * mean_train).max())


def grid_oracle_scores(kind: str, minimize: bool, mean=None, var=None, best_f=None, seed=None):
    """The oracle's acquisition values over the grid (``oracle/gp_oracle.py``) from the given moments, by default scikit-learn's."""
    from oracle import gp_oracle as go

    if mean is None:
        mean, var, best_f = grid_oracle_moments(minimize)
    sign = -1.0 if minimize else 1.0
    if kind in ANALYTIC_KINDS:
        return go.analytic_acq(kind, mean, var, best_f, sign, BETA)
    z = go.sobol_normal_base_samples(N_MC, 1, grid_sampler_seed() if seed is None else seed)[:, 0]
    return go.mc_acq_q1(kind, mean, var, z, best_f, sign, BETA)
