"""Numpy restatement of the Bayesian linear (ARD) surrogate's posterior: ``ARDRegression.predict(return_std=True)`` of scikit-learn
1.7.2 behind the reference's scalers, written from its definition and independent of ``baybe_amd``.

    keep = lambda_ < threshold_lambda
    x~   = (x - lo) / (hi - lo)
    mu~  = x~ . coef_ + intercept_                       (coef_ is exactly 0 at pruned columns)
    var~ = x~[keep]^T sigma_ x~[keep] + 1 / alpha_       (the kept columns are not centred)
    mean = ybar + s mu~,  var = s^2 var~

``bounds`` is what a comparison of two evaluations of these sums is held to: either side's nested sum errs by at most about
(k + 2) eps times the sum of the absolute terms, whatever its order, so
    |mean - ref| <= 4 (k + 4) eps (s (sum_j |coef_j x~_j| + |intercept|) + |ybar|)
    |var  - ref| <= 4 (k + 4) eps s^2 (|x~|^T |Ss| |x~| + 1 / alpha),   Ss = (sigma_ + sigma_^T) / 2.
"""

import numpy as np

EPS = 2.0**-52


def _parts(g: dict, X: np.ndarray):
    keep = np.asarray(g["lambda_"]) < float(g["threshold_lambda"])
    xs = (np.asarray(X, dtype=np.float64) - g["lo"]) / (g["hi"] - g["lo"])
    k = int(keep.sum())
    sigma = np.asarray(g["sigma_"], dtype=np.float64).reshape(k, k)
    return keep, xs, (sigma + sigma.T) / 2.0


def moments(g: dict, X: np.ndarray):
    """(mean [N], var [N]) on the scale of the measurements; ``g`` holds the model arrays and the scaler constants."""
    keep, xs, Ss = _parts(g, X)
    mu = xs @ np.asarray(g["coef_"], dtype=np.float64) + float(g["intercept_"])
    xk = xs[:, keep]
    var = np.einsum("ni,ij,nj->n", xk, Ss, xk) + 1.0 / float(g["alpha_"])
    s = float(g["s"])
    return float(g["ybar"]) + s * mu, s * s * var


def reference_from_sklearn(g: dict):
    """scikit-learn's stored ``predict(return_std=True)`` (standardised units) on the scale of the measurements."""
    s = float(g["s"])
    return float(g["ybar"]) + s * g["pred_mean"], s * s * g["pred_std"] ** 2


def bounds(g: dict, X: np.ndarray):
    """(bound on |mean - ref| [N], bound on |var - ref| [N]) as stated above."""
    keep, xs, Ss = _parts(g, X)
    k = int(keep.sum())
    s = float(g["s"])
    amean = s * (np.abs(xs * np.asarray(g["coef_"])).sum(axis=1) + abs(float(g["intercept_"]))) + abs(float(g["ybar"]))
    xk = np.abs(xs[:, keep])
    avar = s * s * (np.einsum("ni,ij,nj->n", xk, np.abs(Ss), xk) + 1.0 / float(g["alpha_"]))
    return 4 * (k + 4) * EPS * amean, 4 * (k + 4) * EPS * avar


def constant_moments(train_y: np.ndarray):
    """Posterior of the constant-target fallback (``MeanPredictionSurrogate`` on the standardised targets): (mean, var), the same at
    every row."""
    y = np.asarray(train_y, dtype=np.float64).reshape(-1)
    ybar = float(y.mean())
    s = float(y.std(ddof=1)) if y.size > 1 else float("nan")
    if not (s >= 1e-8):
        s = 1.0
    return ybar + s * float(np.mean((y - ybar) / s)), s * s


def fit_reference(train_x, train_y, lo, hi, X, model_params=None):
    """The reference's path end to end with scikit-learn itself: scale, standardise, ``ARDRegression.fit``,
    ``predict(return_std=True)``; (mean [N], var [N], mean at the training rows [n]) on the scale of the measurements."""
    from sklearn.linear_model import ARDRegression

    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    y = np.asarray(train_y, dtype=np.float64).reshape(-1)
    ybar, s = float(y.mean()), float(y.std(ddof=1))
    model = ARDRegression(**(model_params or {})).fit((np.asarray(train_x) - lo) / (hi - lo), (y - ybar) / s)
    mean, std = model.predict((np.asarray(X) - lo) / (hi - lo), return_std=True)
    mean_train = model.predict((np.asarray(train_x) - lo) / (hi - lo))
    return ybar + s * mean, s * s * std**2, ybar + s * mean_train


def best_and_margin(scores: np.ndarray):
    """(first index of the best score, best minus second-best score)."""
    scores = np.asarray(scores, dtype=np.float64)
    order = np.argsort(-scores, kind="stable")
    return int(order[0]), float(scores[order[0]] - scores[order[1]])
