"""Bayesian linear (ARD) surrogate for the HIP path: scikit-learn fits the model on the host, the device evaluates its moments.

``HipBayesianLinearSurrogate`` mirrors ``BayesianLinearSurrogate`` (``baybe/surrogates/linear.py``: scikit-learn's ``ARDRegression``
behind ``IndependentGaussianSurrogate``): ``fit`` is ``Surrogate.fit`` (``surrogates/base.py:387-465``) with the base-class scalers,
neither of which ``linear.py`` overrides - every comp-rep column is min-max scaled over ``searchspace.scaling_bounds``
(``x~ = (x - lo) / (hi - lo)``, a subtraction and a division as the GP path's [UPSTREAM]-tagged ``Normalize`` convention), the targets
are standardised (``Standardize(1)``: Bessel deviation, below 1e-8 it becomes 1) - and ends in
``ARDRegression(**model_params).fit(x~, y~)``, the reference's own call.  That fit stays on the host and is small.  What moves to the
device is everything after it: the reference calls ``model.predict(X, return_std=True)`` over all N candidates
(``np.dot(X, sigma_) * X``: an ``[N, k]`` temporary and N k^2 flops on the host), wraps the result in an MVN and lets BoTorch score it
in chunks; here ``bbh_linear_moments`` goes from the resident candidate matrix to the un-standardised mean and variance of every row
in one pass, and the existing q = 1 scorers and selection kernels take it from there.

The moments are scikit-learn's (1.7.2): with ``keep = lambda_ < threshold_lambda``, ``mu~ = x~ . coef_ + intercept_`` (``coef_`` is
exactly 0 at pruned columns) and ``var~ = x~[keep]^T sigma_ x~[keep] + 1 / alpha_`` - the kept columns are NOT centred, which is
scikit-learn's behaviour and stays.  ``sigma_`` from the Woodbury branch (n < d) is not exactly symmetric; the quadratic form only sees
``(sigma_ + sigma_^T) / 2``.  It comes from ``pinvh`` and may be only positive semi-definite: it is never factorised.

Constant targets (``catch_constant_targets``, ``surrogates/utils.py:27-85``, wrapping ``_fit`` and so seeing the STANDARDISED targets:
one row, or ``std(y~, ddof=1) < 1e-6``) fit no model: the fallback is ``MeanPredictionSurrogate`` (``surrogates/naive.py``), mean
``mean(y~)`` and variance 1 at every row - here a pack without kept columns.

The posterior is an independent Gaussian per row, for t-batches of ONE point (``IndependentGaussianSurrogate._posterior``,
``surrogates/base.py:484-503``): a joint q > 1 evaluation raises ``IncompatibleSurrogateError`` in the reference, so a greedy batch of
2 or any pending experiment fails there, and fails here - before anything is fitted.
"""

from __future__ import annotations

from typing import ClassVar

import attrs
import numpy as np
import pandas as pd
from attrs import field

from baybe_amd.engine import GreedyResult, HipGP, sobol_normal_base_samples
from baybe_amd.exceptions import IncompatibilityError, IncompatibleSurrogateError, ModelNotTrainedError
from baybe_amd.forest import _BOOL, _FLOAT, _INT, _matches, refuse_continuous
from baybe_amd.scoring import HipSingleTargetAcq, refuse_shard
from baybe_amd.surrogates import (
    _availability_property,
    _frame_hash,
    _objective_key,
    _target_sign,
    modeled_quantities,
    pre_transformed,
)

CONSTANT_TARGET_STD = 1e-6  # catch_constant_targets(std_threshold=1e-6)
MIN_STDV = 1e-8  # Standardize: a deviation below this becomes 1
MAX_KEPT = 512  # kept columns bbh_linear_moments takes
REGISTER_MAX_KEPT = 32  # ... in its register form
AUTO_REGISTER_MAX_KEPT = 16  # ... and up to where form "auto" takes the register form (the measured crossover)

JOINT_TEXT = ("cannot be used for joint posterior evaluation: its posterior is an independent Gaussian per point, so batches of more "
              "than one point and pending experiments are not supported (as for the reference's BayesianLinearSurrogate)")



def refuse_joint(name: str, batch_size: int, n_pend: int) -> None:
    """An independent Gaussian per point has no joint posterior (surrogates/base.py:484-503): one point, nothing pending."""
    if batch_size != 1 or n_pend > 0:
        raise IncompatibleSurrogateError(f"'{name}' {JOINT_TEXT}.")


def shard_text(name: str) -> str:
    return f"Row shards are not on the HIP path of '{name}'; score the linear model on one device."


# ---- model_params: make_dict_validator(_ARDRegressionParams) without cattrs ---------------------------------------------------------
_ARD_PARAMS = {  # linear.py:20-36
    "max_iter": (_INT,),
    "tol": (_FLOAT,),
    "alpha_1": (_FLOAT,),
    "alpha_2": (_FLOAT,),
    "lambda_1": (_FLOAT,),
    "lambda_2": (_FLOAT,),
    "compute_score": (_BOOL,),
    "threshold_lambda": (_FLOAT,),
    "fit_intercept": (_BOOL,),
    "copy_X": (_BOOL,),
    "verbose": (_BOOL,),
}


def validate_model_params(_, attribute, value) -> None:
    """The reference's validator: unknown keys and values outside the declared types fail with one ``TypeError``."""
    for key, val in value.items():
        specs = _ARD_PARAMS.get(key)
        if specs is None or not any(_matches(val, s) for s in specs):
            raise TypeError(f"The provided dictionary for '{attribute.name}' is invalid.")


# ---- packing ------------------------------------------------------------------------------------------------------------------------
def pack_linear(model, lo, hi) -> dict:
    """What the device reads of a fitted ``ARDRegression`` (anything with ``lambda_``, ``threshold_lambda``, ``coef_``, ``intercept_``,
    ``sigma_``, ``alpha_``) and the scaler constants ``lo`` / ``hi`` ``[d]``: per kept column (``lambda_ < threshold_lambda``) its
    comp-rep column ``cols`` (int32), ``lo``, ``range = hi - lo`` and ``coef``, and ONE ``[k, k]`` matrix ``T`` with
    ``T[i][i] = Ss[i][i]``, ``T[i][j] = 2 Ss[i][j]`` for ``j < i`` and 0 above the diagonal, ``Ss = (sigma_ + sigma_^T) / 2`` - so that
    ``x~^T sigma_ x~ = x~^T T x~`` with work on and below the diagonal only.  Pure numpy."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    keep = np.asarray(model.lambda_, dtype=np.float64) < float(model.threshold_lambda)
    if keep.shape != lo.shape or lo.shape != hi.shape:
        raise ValueError("pack_linear: lambda_, lo and hi must have one entry per column")
    cols = np.nonzero(keep)[0].astype(np.int32)
    k = len(cols)
    sigma = np.asarray(model.sigma_, dtype=np.float64).reshape(k, k)
    Ss = (sigma + sigma.T) / 2.0
    T = np.tril(2.0 * Ss, -1) + np.diag(np.diag(Ss))
    return {"cols": cols, "lo": lo[cols].copy(), "range": (hi - lo)[cols], "coef": np.asarray(model.coef_, dtype=np.float64).reshape(-1)[cols].copy(),
            "T": np.ascontiguousarray(T), "intercept": float(model.intercept_), "inv_alpha": 1.0 / float(model.alpha_)}


def constant_linear(value: float) -> dict:
    """The model of constant training targets: no kept column, mean ``value`` and variance 1 (on the standardised scale)."""
    return {"cols": np.zeros(0, dtype=np.int32), "lo": np.zeros(0), "range": np.zeros(0), "coef": np.zeros(0), "T": np.zeros((0, 0)),
            "intercept": float(value), "inv_alpha": 1.0}


def check_packed_linear(packed: dict, d: int) -> None:
    """What the kernels rely on, checked before anything is uploaded: tables of one length k <= 512, columns inside ``[0, d)``, every
    entry finite, ``range > 0``, ``T`` lower triangular (its diagonal included)."""
    cols = np.asarray(packed["cols"])
    k = int(cols.shape[0])
    if cols.ndim != 1 or cols.dtype != np.int32:
        raise ValueError("packed linear model: cols must be a one-dimensional int32 array")
    if k > MAX_KEPT:
        raise ValueError(f"packed linear model: {k} kept columns, the device pass takes at most {MAX_KEPT}")
    for key in ("lo", "range", "coef"):
        if np.asarray(packed[key]).shape != (k,):
            raise ValueError(f"packed linear model: '{key}' must have one entry per kept column")
    T = np.asarray(packed["T"])
    if T.shape != (k, k):
        raise ValueError("packed linear model: T must be [k, k]")
    if (cols < 0).any() or (cols >= d).any():
        raise ValueError(f"packed linear model: a kept column lies outside the {d} columns")
    tables = [np.asarray(packed[key], dtype=np.float64) for key in ("lo", "range", "coef", "T")]
    scalars = np.array([packed["intercept"], packed["inv_alpha"]], dtype=np.float64)
    if not all(np.isfinite(t).all() for t in tables) or not np.isfinite(scalars).all():
        raise ValueError("packed linear model: a table holds a value that is not finite")
    if (np.asarray(packed["range"]) <= 0.0).any():
        raise ValueError("packed linear model: the range hi - lo of a kept column is not positive")
    if np.triu(T, 1).any():
        raise ValueError("packed linear model: T must be lower triangular (strictly lower triangle plus diagonal)")


# ---- the device-side model -------------------------------------------------------------------------------------------------------------
class HipLinearEngine(HipGP):
    """The library handle of a Bayesian linear surrogate plus its packed tables on the device.  ``posterior`` answers with the
    predictive moments, so the recommender's analytic and read-back paths drive it like a GP engine; ``mc_acq``, ``analytic_acq``,
    ``argmax`` and ``topk`` are the parent's and take the moments as they are."""

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.packed = None
        self.d = 0
        self.form = "auto"
        self._L = None
        self._finite = None  # (weak reference to a device matrix found free of NaN and infinities, its version counter)

    def __getstate__(self):
        st = super().__getstate__()
        st["linear"] = (self.packed, self.d, self.form)
        return st

    def __setstate__(self, st):
        super().__setstate__(st)
        self.packed, self.d, self.form = st["linear"]
        self._L = self._finite = None
        self._restorable = False  # (no GP model to rebuild ...)
        self._copied = True  # (... a copied / unpickled engine acquires its handle on first use and uploads its tables again)

    @property
    def _h(self):
        """The device handle; None once the engine is closed, as for the parent."""
        if self._handle is None and getattr(self, "_copied", False):
            from baybe_amd.engine import _acquire_handle, _pool_key

            self._copied = False
            self._handle = _acquire_handle(self._lib, self.device)
            self._pool_key = _pool_key(self.device)
        return self._handle

    def close(self):
        super().close()
        self._copied = False
        self._L = self._finite = None

    def set_linear(self, packed: dict, d: int, ybar: float = 0.0, ysd: float = 1.0) -> None:
        check_packed_linear(packed, d)
        self.packed, self.d, self.ybar, self.ysd = packed, int(d), float(ybar), float(ysd)
        self._L = self.linear_upload(packed)

    @property
    def linear(self) -> dict:
        if self.packed is None:
            raise ModelNotTrainedError("The surrogate must be trained before a posterior can be computed.")
        if self._L is None:
            self._L = self.linear_upload(self.packed)
        return self._L

    def _as_dev(self, X):
        """Rows as an fp64 device matrix, refused if they hold a value that is not finite.  A host array is looked at on the host before
        it is copied, every time.  A device tensor is looked at on the device; only a tensor the caller keeps alive - the recommender's
        resident candidate matrix - is remembered, by identity and version counter, so that the passes of one recommendation over it pay
        for one look."""
        torch = self._torch()
        if isinstance(X, np.ndarray):
            X = np.ascontiguousarray(X, dtype=np.float64)
            if not np.isfinite(X).all():
                raise ValueError("Non-finite values among the candidate rows: the linear surrogate needs finite inputs.")
            X, checked = torch.from_numpy(X), True
        else:
            checked = False
        given = X
        if X.dtype != torch.float64:
            X = X.to(torch.float64)
        X = X.to(self._dev())
        if X.dim() != 2 or X.shape[1] < self.d:
            raise ValueError("candidates must be [N, d]")
        if X.stride(1) != 1:
            X = X.contiguous()
        if X.shape[0] == 1 and X.stride(0) < X.shape[1]:
            X = X.as_strided(X.shape, (X.shape[1], 1))
        if not checked:
            self._refuse_non_finite(X, remember=X is given)
        return X

    def _refuse_non_finite(self, X, remember: bool) -> None:
        seen = self._finite
        if seen is not None and seen[0]() is X and seen[1] == X._version:
            return  # the very tensor that was looked at, alive since and not written to
        if not bool(self._torch().isfinite(X).all()):
            raise ValueError("Non-finite values among the candidate rows: the linear surrogate needs finite inputs.")
        if remember:  # (a tensor made inside _as_dev dies with the call: its address says nothing about the next one)
            import weakref

            self._finite = (weakref.ref(X), X._version)

    def posterior(self, X, unfused: bool = False, out=None, form=None):
        """(predictive mean, predictive variance) on the scale of the measurements, device tensors [N]."""
        return self.linear_moments(self.linear, self._as_dev(X), self.ybar, self.ysd, self.form if form is None else form)

    def best_f(self, sign: float = 1.0, objective=None) -> float:
        """max_i objective(mean at training row i) (``acquisition/_builder.py:141-161``); ``objective``: an ``ObjectiveProgram`` in place
        of ``sign``."""
        mean, _ = self.posterior(self._X_train)
        mean = mean.cpu().numpy()
        if objective is not None:
            return float(objective.apply(mean).max())
        return float((float(sign) * mean).max())


# ---- the acquisition scorer the recommender drives -----------------------------------------------------------------------------------
class HipLinearAcq:
    """MC acquisition functions under the independent Gaussian posterior of the linear surrogate, in the slot and with the surface of
    the recommender's other device scorers (``greedy`` / ``prepare`` / ``score`` / ``outputs``): q = 1 values through
    ``eng.mc_acq(kind, mean, var, z, ...)`` with ``sobol_normal_base_samples(S, 1, seed)``; first-index argmax."""

    def __init__(self, surrogate, kind: str, sign: float, best_f: float, n_mc_samples: int, beta: float = 0.2, objective=None):
        self.name = type(surrogate).__name__
        self.engine = surrogate.engine
        self.kind, self.sign, self.best_f, self.S, self.beta = kind, float(sign), float(best_f), int(n_mc_samples), float(beta)
        self.objective = objective
        self._z = None

    def prepare(self, seed: int, X_pending=None) -> None:
        refuse_joint(self.name, 1, 0 if X_pending is None else len(X_pending))
        self._z = sobol_normal_base_samples(self.S, 1, seed)[:, 0]

    def score(self, Xd, alive=None):
        eng = self.engine
        mean, var = eng.posterior(Xd)
        okw = {} if self.objective is None else {"objective": self.objective}
        return eng.mc_acq(self.kind, mean, var, self._z, self.best_f, self.sign, self.beta, alive=alive, **okw)

    def greedy(self, Xd, batch_size: int, seed: int, X_pending=None, alive=None) -> GreedyResult:
        if batch_size != 1:
            raise IncompatibleSurrogateError(f"'{self.name}' {JOINT_TEXT}.")
        self.prepare(seed, X_pending)
        val, idx = self.engine.argmax(self.score(Xd, alive))
        return GreedyResult([int(idx)], [float(val)])

    # ---- the recommender's surface (``baybe_amd.scoring``): ONE sampler seed per call ----------------------------------------------
    supports_continuous = False

    @staticmethod
    def check_request(batch_size, n_pend, acqf=None, program=None, model=None) -> None:
        refuse_joint(type(model).__name__, batch_size, n_pend)

    def select(self, X, q, *, seeds, X_pending=None, alive=None, shard=None) -> GreedyResult:
        refuse_shard(shard, shard_text(self.name))
        return self.greedy(X, q, seeds(), X_pending, alive)

    def values(self, X, *, seeds, X_pending=None):
        self.prepare(seeds(), X_pending)
        return self.score(self.engine._as_dev(X))

    def joint_value(self, batch, *, seeds, X_pending=None) -> float:
        refuse_joint(self.name, len(batch), 0)
        return float(self.values(batch, seeds=seeds, X_pending=X_pending).cpu().numpy()[0])


class HipLinearAnalytic(HipSingleTargetAcq):
    """The analytic acquisition functions on the linear model's moments: ``HipSingleTargetAcq`` under the one-point rule."""

    supports_continuous = False
    check_request = staticmethod(HipLinearAcq.check_request)

    def __init__(self, surrogate, acqf, sign: float, best_f: float, program=None):
        super().__init__(surrogate.engine, acqf, sign, best_f, program)
        self.name = type(surrogate).__name__

    def joint_value(self, batch, *, seeds, X_pending=None) -> float:
        refuse_joint(self.name, len(batch), 0)
        return super().joint_value(batch, seeds=seeds, X_pending=X_pending)


# ---- the surrogate -----------------------------------------------------------------------------------------------------------------------
def scale_inputs(x: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """``Normalize`` over the scaling bounds: ``(x - lo) / (hi - lo)``."""
    return (np.asarray(x, dtype=np.float64) - lo) / (hi - lo)


def standardize_targets(y: np.ndarray):
    """``Standardize(1)``: (y~, ybar, s) with the Bessel deviation; a deviation below 1e-8 (or of a single value) becomes 1."""
    values = np.array(y, dtype=np.float64).ravel()
    centre = float(np.mean(values))
    spread = float(np.std(values, ddof=1)) if values.size >= 2 else 1.0
    if not spread >= MIN_STDV:  # (a NaN deviation falls here as well)
        spread = 1.0
    return (values - centre) / spread, centre, spread


def is_constant_target(y_std: np.ndarray) -> bool:
    """``catch_constant_targets`` on the standardised targets: one value, or an (unbiased) standard deviation below 1e-6."""
    y_std = np.asarray(y_std, dtype=np.float64)
    return y_std.size == 1 or float(np.std(y_std, ddof=1)) < CONSTANT_TARGET_STD


def fit_linear(train_x: np.ndarray, train_y: np.ndarray, lo: np.ndarray, hi: np.ndarray, model_params: dict):
    """(packed model, ybar, s, the scikit-learn model or None): the host-side fit on scaled inputs and standardised targets."""
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    y_std, ybar, s = standardize_targets(train_y)
    if is_constant_target(y_std):
        return constant_linear(float(np.mean(y_std))), ybar, s, None
    if not ((hi - lo) > 0.0).all():
        raise ValueError("The scaling bounds of a column have no extent: the inputs cannot be min-max scaled.")
    from sklearn.linear_model import ARDRegression

    model = ARDRegression(**model_params)
    model.fit(scale_inputs(train_x, lo, hi), y_std)
    return pack_linear(model, lo, hi), ybar, s, model


class HipLinearSurrogateImpl:
    """Behaviour of the Bayesian linear surrogate scored on an MI355X (no fields: ``attrs.make_class`` attaches them, below for the
    stand-alone class and in ``baybe_amd.plugin.make_baybe_linear_surrogate`` on top of BayBE's ``Surrogate``)."""

    __slots__ = ()

    supports_transfer_learning: ClassVar[bool] = False
    supports_multi_output: ClassVar[bool] = False
    is_independent_gaussian: ClassVar[bool] = True
    is_available = _availability_property()

    def fit(self, searchspace, objective, measurements: pd.DataFrame) -> None:
        quantities = modeled_quantities(objective)
        if len(quantities) > 1 or getattr(objective, "is_multi_output", False):
            raise IncompatibleSurrogateError(
                f"You attempted to train a single-output surrogate in a "
                f"{len(objective.targets)}-target multi-output context. Either use "
                f"a proper multi-output surrogate or consider explicitly "
                f"replicating the current surrogate model using its "
                f"'.replicate' method."
            )
        n_tasks = int(getattr(searchspace, "n_tasks", 1))
        bounds = np.asarray(searchspace.scaling_bounds.to_numpy(), dtype=np.float64)
        # unchanged context -> no refit, keyed like the forest's cache: the encoding, the target definition, the parameters, the measurements
        mhash = (
            tuple(searchspace.comp_rep_columns),
            bounds.tobytes(),
            getattr(searchspace, "task_idx", None),
            n_tasks,
            _objective_key(objective),
            repr(sorted(self.model_params.items(), key=lambda kv: kv[0])),
            _frame_hash(measurements),
        )
        if self._engine is not None and self._engine.packed is not None and mhash == self._measurements_hash:
            self._searchspace, self._objective = searchspace, objective
            return
        refuse_task_parameters(searchspace, type(self).__name__)
        refuse_continuous(searchspace)
        target = quantities[0]
        needs = getattr(objective, "_model_quantities_to_target_names", None)
        names = list(needs[target.name]) if needs is not None else [target.name]
        if any(pd.isna(measurements[nm].to_numpy()).any() for nm in names):
            raise ValueError(f"Missing target values are not supported: {[t.name for t in objective.targets]}")
        comp = searchspace.transform(measurements, allow_extra=True)
        train_x = np.ascontiguousarray(comp.to_numpy(dtype=np.float64))
        train_y = pre_transformed(objective, measurements)[target.name].to_numpy(dtype=np.float64)
        if not np.isfinite(train_x).all():
            raise ValueError("Non-finite values among the training rows: the linear surrogate needs finite inputs.")
        packed, ybar, s, model = fit_linear(train_x, train_y, bounds[0], bounds[1], self.model_params)
        check_packed_linear(packed, train_x.shape[1])
        if self._engine is None:
            self._engine = HipLinearEngine(self.device)
        self._engine._X_train, self._engine._y_train = train_x, train_y
        self._engine.set_linear(packed, train_x.shape[1], ybar, s)
        self._model = model
        self._searchspace, self._objective, self._measurements_hash = searchspace, objective, mhash

    def to_botorch(self):
        raise IncompatibilityError(
            "HipBayesianLinearSurrogate does not wrap a BoTorch model: the predictive moments and the acquisition "
            "are evaluated by libbaybe_hip. Use posterior_mean_var() / posterior_stats(), or a "
            "BotorchRecommender with baybe's BayesianLinearSurrogate for BoTorch-only features."
        )

    # ---- abstract hooks of baybe.surrogates.base.Surrogate (base.py:274-306, 467-469) ------------------------
    def _fit(self, train_x, train_y) -> None:
        raise NotImplementedError("HipBayesianLinearSurrogate.fit() scales, fits, packs and uploads the model itself.")

    def _posterior(self, candidates_comp_scaled, /):
        raise IncompatibilityError(
            "HipBayesianLinearSurrogate builds no BoTorch posterior: the independent Gaussian moments are evaluated on the device. "
            "Use posterior_mean_var() / posterior_stats()."
        )

    @property
    def engine(self):
        if self._engine is None or self._objective is None:
            raise ModelNotTrainedError("The surrogate must be trained before a posterior can be computed.")
        return self._engine

    @property
    def sign(self) -> float:
        return _target_sign(modeled_quantities(self._objective)[0])

    def posterior_mean_var(self, candidates_comp):
        """(predictive mean, predictive variance) on the scale of the measurements as device tensors [N]."""
        return self.engine.posterior(candidates_comp)

    def posterior_stats(self, candidates: pd.DataFrame, stats=("mean", "std")) -> pd.DataFrame:
        """``Surrogate.posterior_stats`` (surrogates/base.py:308-384): ``<target>_<stat>`` columns, Gaussian quantiles included."""
        eng = self.engine
        for s in (x for x in stats if isinstance(x, float)):
            if not 0.0 < s < 1.0:
                raise ValueError(
                    f"Posterior quantile statistics can only be computed for quantiles between 0 and 1 "
                    f"(non-inclusive). Provided value: '{s}' as part of '{stats=}'."
                )
        for s in stats:
            if not isinstance(s, float) and s not in ("mean", "std", "var"):
                raise TypeError(f"The HIP posterior does not support the statistic '{s}'.")
        comp = self._searchspace.transform(candidates, allow_extra=True)
        mean, var = eng.posterior(np.ascontiguousarray(comp.to_numpy(dtype=np.float64)))
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        name = modeled_quantities(self._objective)[0].name
        out = pd.DataFrame(index=candidates.index)
        for s in stats:
            if isinstance(s, float):
                from scipy.stats import norm

                out[f"{name}_Q_{s}"] = mean + np.sqrt(var) * norm.ppf(s)
            else:
                out[f"{name}_{s}"] = {"mean": mean, "std": np.sqrt(var), "var": var}[s]
        return out


def refuse_task_parameters(searchspace, name: str) -> None:
    """``Surrogate.fit`` (``surrogates/base.py:396-402``): no transfer learning."""
    if int(getattr(searchspace, "n_tasks", 1)) > 1:
        raise ValueError(
            f"The search space contains task parameters but the selected "
            f"surrogate model type ({name}) does not "
            f"support transfer learning."
        )


def linear_surrogate_fields(with_runtime_state: bool = True) -> dict:
    """attrs fields of the linear surrogate.  ``with_runtime_state=False`` leaves out the fields BayBE's ``Surrogate`` base already
    declares (``surrogates/base.py:93-103``)."""
    f = {
        "model_params": field(factory=dict, converter=dict, validator=validate_model_params),
        "device": field(default=0),  # HIP device ordinal
        "_engine": field(init=False, default=None, eq=False, repr=False),
        "_model": field(init=False, default=None, eq=False, repr=False),  # the fitted ARDRegression (None: constant targets)
    }
    if with_runtime_state:
        for name in ("_searchspace", "_objective", "_measurements_hash"):
            f[name] = field(init=False, default=None, eq=False, repr=False)
    return f


HipBayesianLinearSurrogate = attrs.make_class("HipBayesianLinearSurrogate", linear_surrogate_fields(), bases=(HipLinearSurrogateImpl,),
                                              slots=True)
HipBayesianLinearSurrogate.__doc__ = "A Bayesian linear (ARD) surrogate scored on an MI355X (stand-alone class)."
HipBayesianLinearSurrogate.__module__ = __name__
