"""Random forest surrogate for the HIP path: scikit-learn builds the trees on the host, the device walks them.

``HipRandomForestSurrogate`` mirrors ``RandomForestSurrogate`` (``baybe/surrogates/random_forest.py``): ``fit`` is
``Surrogate.fit`` (``surrogates/base.py:387-465``) with the forest's overrides - no input scaler, no output scaler - and ends in
``sklearn.ensemble.RandomForestRegressor(**model_params).fit(train_x, train_y)``, the reference's own call with its draws from
``np.random``.  That fit stays on the host and is the floor of a forest ``recommend()``, as it is in the reference (354 ms for
100 trees on 512 x 20 training rows on one core, ``profiles/forest_pass.json``; the device passes after it take milliseconds).
What moves to the device is everything after it: the reference calls ``predictor.predict(candidates)`` once per tree, stacks an
``[n_estimators, N]`` fp64 matrix, wraps it into an ``EnsemblePosterior`` and lets BoTorch gather rows of it per MC sample; here
the trees are packed into flat node tables once per fit (``pack_forest``) and ``bbh_forest_moments`` / ``bbh_forest_mc_acq`` go
from candidates to moments / acquisition values in one pass, without the matrix.

A prediction equals ``estimator.predict`` bit for bit: the row is cast to float32 and goes left iff
``float64(x32[feature]) <= threshold`` (``sklearn/tree/_tree.pyx``: ``X`` is converted to float32, thresholds are float64).
Missing values are not routed: NaN in training rows or candidates is refused.

Constant targets (one value, or ``torch.std < 1e-6``: ``catch_constant_targets``, ``surrogates/utils.py:27-85``) fit no forest: the
model is ONE single-leaf tree holding ``mean(train_y)`` - the mean of the reference's ``MeanPredictionSurrogate`` fallback
(``surrogates/naive.py:33-46``), whose posterior is that mean with the same constant variance (1) at every candidate; the one-member
ensemble has variance 0.  Either way every candidate has the same posterior, every acquisition value ties across all candidates and
the first index wins on both sides; the values themselves (not the picks) differ from the reference's Gaussian fallback.
"""

from __future__ import annotations

from typing import ClassVar

import attrs
import numpy as np
import pandas as pd
from attrs import field

from baybe_amd.engine import GreedyResult, HipGP
from baybe_amd.exceptions import IncompatibilityError, IncompatibleSurrogateError, ModelNotTrainedError
from baybe_amd.scoring import check_joint_batch, refuse_shard
from baybe_amd.surrogates import (
    _availability_property,
    _frame_hash,
    _objective_key,
    _target_sign,
    modeled_quantities,
    pre_transformed,
)

CONSTANT_TARGET_STD = 1e-6  # catch_constant_targets(std_threshold=1e-6)

# ---- model_params: make_dict_validator(_RandomForestRegressorParams) without cattrs ------------------------------------------------
_INT, _FLOAT, _BOOL, _NONE, _ANY_ARRAY, _RANDOM_STATE = "int", "float", "bool", "none", "array", "random_state"
_FOREST_PARAMS = {  # random_forest.py:27-50
    "n_estimators": (_INT,),
    "criterion": (("squared_error", "absolute_error", "friedman_mse", "poisson"),),
    "max_depth": (_INT,),
    "min_samples_split": (_INT, _FLOAT),
    "min_samples_leaf": (_INT, _FLOAT),
    "min_weight_fraction_leaf": (_FLOAT,),
    "max_features": (("sqrt", "log2"), _INT, _FLOAT, _NONE),
    "max_leaf_nodes": (_INT, _NONE),
    "min_impurity_decrease": (_FLOAT,),
    "bootstrap": (_BOOL,),
    "oob_score": (_BOOL,),
    "n_jobs": (_INT, _NONE),
    "random_state": (_INT, _RANDOM_STATE, _NONE),
    "verbose": (_INT,),
    "warm_start": (_BOOL,),
    "ccp_alpha": (_FLOAT,),
    "max_samples": (_INT, _FLOAT, _NONE),
    "monotonic_cst": (_ANY_ARRAY, _INT, _NONE),
}


def _matches(value, spec) -> bool:
    if isinstance(spec, tuple):  # a Literal
        return isinstance(value, str) and value in spec
    if spec == _INT:  # a real int: bool is a subclass of int and is not meant
        return isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_))
    if spec == _FLOAT:
        return isinstance(value, (float, np.floating))
    if spec == _BOOL:
        return isinstance(value, (bool, np.bool_))
    if spec == _NONE:
        return value is None
    if spec == _RANDOM_STATE:
        return isinstance(value, np.random.RandomState)
    if spec == _ANY_ARRAY:
        return isinstance(value, (list, tuple, np.ndarray))
    return False


def validate_model_params(_, attribute, value) -> None:
    """The reference's validator: unknown keys and values outside the declared types fail with one ``TypeError``."""
    for key, val in value.items():
        specs = _FOREST_PARAMS.get(key)
        if specs is None or not any(_matches(val, s) for s in specs):
            raise TypeError(f"The provided dictionary for '{attribute.name}' is invalid.")


# ---- packing ------------------------------------------------------------------------------------------------------------------------
def pack_forest(estimators) -> dict:
    """Flat node arrays of fitted trees (anything with a ``tree_`` holding ``children_left``, ``children_right``, ``feature``,
    ``threshold``, ``value``): ``offsets [T + 1]`` int64 (first node of every tree), ``children_left`` / ``children_right`` /
    ``feature`` int32 and ``threshold`` / ``value`` fp64 over all nodes, trees in order, children counted from their tree's first
    node as scikit-learn counts them.  Nothing is assumed about where a child sits (``max_leaf_nodes`` grows trees best-first:
    the left child is not ``node + 1``).  Pure numpy."""
    left, right, feat, thr, val, offsets = [], [], [], [], [], [0]
    for est in estimators:
        tree = getattr(est, "tree_", est)
        n = int(np.asarray(tree.children_left).shape[0])
        left.append(np.asarray(tree.children_left, dtype=np.int32).reshape(n))
        right.append(np.asarray(tree.children_right, dtype=np.int32).reshape(n))
        feat.append(np.asarray(tree.feature, dtype=np.int32).reshape(n))
        thr.append(np.asarray(tree.threshold, dtype=np.float64).reshape(n))
        value = np.asarray(tree.value, dtype=np.float64)
        val.append(np.ascontiguousarray(value[:, 0, 0] if value.ndim == 3 else value.reshape(n)))
        offsets.append(offsets[-1] + n)
    if not left:
        raise ValueError("pack_forest needs at least one tree")
    return {
        "offsets": np.asarray(offsets, dtype=np.int64),
        "children_left": np.concatenate(left), "children_right": np.concatenate(right), "feature": np.concatenate(feat),
        "threshold": np.concatenate(thr), "value": np.concatenate(val),
    }


def unpack_forest(packed: dict) -> list:
    """The per-tree arrays ``pack_forest`` was given, as dicts (views of the packed arrays)."""
    off = packed["offsets"]
    keys = ("children_left", "children_right", "feature", "threshold", "value")
    return [{k: packed[k][off[t]:off[t + 1]] for k in keys} for t in range(len(off) - 1)]


def single_leaf_forest(value: float) -> dict:
    """One tree that is one leaf: the model of constant training targets."""
    return {"offsets": np.array([0, 1], dtype=np.int64), "children_left": np.array([-1], dtype=np.int32),
            "children_right": np.array([-1], dtype=np.int32), "feature": np.array([-2], dtype=np.int32),
            "threshold": np.array([-2.0]), "value": np.array([float(value)])}


def check_packed(packed: dict, d: int) -> None:
    """What the kernels rely on, checked before anything is uploaded: every inner node has two children inside its own tree and a
    feature below ``d``; a node is a leaf on both sides or on neither."""
    off = np.asarray(packed["offsets"], dtype=np.int64)
    left, right, feat = packed["children_left"], packed["children_right"], packed["feature"]
    n = len(left)
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != n or (np.diff(off) < 1).any():
        raise ValueError("packed forest: offsets must rise from 0 to the node count, one node per tree at least")
    if not (len(right) == len(feat) == len(packed["threshold"]) == len(packed["value"]) == n):
        raise ValueError("packed forest: the node arrays differ in length")
    size = np.repeat(np.diff(off), np.diff(off))
    inner = left >= 0
    if ((right >= 0) != inner).any():
        raise ValueError("packed forest: a node has one child only")
    if (left[inner] >= size[inner]).any() or (right[inner] >= size[inner]).any():
        raise ValueError("packed forest: a child lies outside its tree")
    if (feat[inner] < 0).any() or (feat[inner] >= d).any():
        raise ValueError(f"packed forest: a split feature lies outside the {d} columns")
    if np.isnan(packed["threshold"][inner]).any() or np.isnan(packed["value"][~inner]).any():
        raise ValueError("packed forest: NaN among the thresholds or leaf values")


# ---- which tree each MC sample reads -------------------------------------------------------------------------------------------------
def ensemble_member_indices(S: int, T: int, seed: int) -> np.ndarray:
    """The ensemble member each of the ``S`` MC samples reads, ``[S]`` int64 in ``[0, T)``: BoTorch's ``IndexSampler`` draws them from
    a generator seeded with the sampler seed.

    [UPSTREAM]-unpinned: the draw's spelling differs between BoTorch versions (``torch.randint(0, T, (S,))`` in older ones,
    ``torch.multinomial`` over uniform weights in newer ones) and BoTorch is not importable where this was written; this is the
    ``randint`` form.  It is the ONE place that decides the assignment - everything downstream consumes only
    ``counts[t] = #{s : idx_s = t}`` (``ensemble_member_counts``), so a correction touches this function alone.

    The numbers are those of ``torch.manual_seed(seed); torch.randint(0, T, (S,))`` under ``torch.random.fork_rng()``
    (``tests/test_forest_cpu.py`` compares the two), drawn from a private CPU generator seeded with ``seed``: the same Mersenne
    twister stream, with no global generator of any device saved, reseeded or restored."""
    import torch

    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return torch.randint(0, int(T), (int(S),), generator=gen).numpy().astype(np.int64)


def ensemble_member_counts(S: int, T: int, seed: int) -> np.ndarray:
    """``counts[t]`` = number of the ``S`` MC samples that read tree ``t`` (int32, sums to ``S``)."""
    return np.bincount(ensemble_member_indices(S, T, seed), minlength=int(T)).astype(np.int32)


# ---- the device-side forest ------------------------------------------------------------------------------------------------------------
class HipForestEngine(HipGP):
    """The library handle of a forest surrogate plus its node tables on the device.  ``posterior`` answers with the ensemble moments,
    so the recommender's analytic and read-back paths drive it like a GP engine."""

    def __init__(self, device: int = 0):
        super().__init__(device)
        self.packed = None
        self.d = 0
        self._F = None
        self._nan_free = None  # (weak reference to a device matrix found free of NaN, its version counter)

    def __getstate__(self):
        st = super().__getstate__()
        st["forest"] = (self.packed, self.d)
        return st

    def __setstate__(self, st):
        super().__setstate__(st)
        self.packed, self.d = st["forest"]
        self._F = self._nan_free = None
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
        self._F = self._nan_free = None

    def set_forest(self, packed: dict, d: int) -> None:
        check_packed(packed, d)
        self.packed, self.d = packed, int(d)
        self._F = self.forest_upload(packed, d)

    @property
    def forest(self) -> dict:
        if self.packed is None:
            raise ModelNotTrainedError("The surrogate must be trained before a posterior can be computed.")
        if self._F is None:
            self._F = self.forest_upload(self.packed, self.d)
        return self._F

    @property
    def n_trees(self) -> int:
        return int(self.forest["T"])

    def _as_dev(self, X):
        """Rows as an fp64 device matrix, refused if they hold NaN (missing-value routing is not supported).  A host array is looked
        at on the host before it is copied, every time.  A device tensor is looked at on the device; only a tensor the caller keeps
        alive - the recommender's resident candidate matrix - is remembered, by identity and version counter, so that the passes of
        one recommendation over it pay for one look."""
        torch = self._torch()
        if isinstance(X, np.ndarray):
            X = np.ascontiguousarray(X, dtype=np.float64)
            if np.isnan(X).any():
                raise ValueError("NaN among the candidate rows: the forest surrogate does not route missing values.")
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
            self._refuse_nan(X, remember=X is given)
        return X

    def _refuse_nan(self, X, remember: bool) -> None:
        seen = self._nan_free
        if seen is not None and seen[0]() is X and seen[1] == X._version:
            return  # the very tensor that was looked at, alive since and not written to
        if bool(self._torch().isnan(X).any()):
            raise ValueError("NaN among the candidate rows: the forest surrogate does not route missing values.")
        if remember:  # (a tensor made inside _as_dev dies with the call: its address says nothing about the next one)
            import weakref

            self._nan_free = (weakref.ref(X), X._version)

    def predict(self, X):
        """Per-tree predictions ``[T, n]`` (device tensor) of a SMALL row set."""
        return self.forest_predict(self.forest, self._as_dev(X))

    def posterior(self, X, unfused: bool = False, out=None):
        """(mean, unbiased variance) over the trees, device tensors [N]: ``EnsemblePosterior.mean`` / ``.variance``."""
        return self.forest_moments(self.forest, self._as_dev(X))

    def best_f(self, sign: float = 1.0, objective=None) -> float:
        """max_i sign * mean_t P_t(x_i) over the training inputs (``acquisition/_builder.py:141-161``)."""
        mean, _ = self.posterior(self._X_train)
        return float((float(sign) * mean).max().item())


# ---- the acquisition scorer the recommender drives -----------------------------------------------------------------------------------
def shard_text(name: str) -> str:
    return f"Row shards are not on the HIP path of '{name}'; score the forest on one device."


class HipForestAcq:
    """MC acquisition functions under the forest's ensemble posterior, in the slot and with the surface of the recommender's other
    device scorers (``baybe_amd.scoring``, over ``greedy`` / ``prepare`` / ``score``).  One sampler seed per recommendation; the greedy loop keeps the member
    counts fixed across its steps (same sampler, same base samples), appends each pick's per-tree predictions to the pending block
    and masks the pick out; first-index argmax."""

    def __init__(self, surrogate, kind: str, sign: float, best_f: float, n_mc_samples: int, beta: float = 0.2):
        self.name = type(surrogate).__name__
        self.engine = surrogate.engine
        self.kind, self.sign, self.best_f, self.S, self.beta = kind, float(sign), float(best_f), int(n_mc_samples), float(beta)
        self._counts = self._order = self._pend = None

    def prepare(self, seed: int, X_pending=None) -> None:
        eng = self.engine
        torch = eng._torch()
        counts = ensemble_member_counts(self.S, eng.n_trees, seed)
        self.counts_host = counts
        self._counts = torch.from_numpy(counts).to(eng._dev())
        self._order = torch.from_numpy(np.nonzero(counts)[0].astype(np.int32)).to(eng._dev())
        self._pend = None
        if X_pending is not None and len(X_pending):
            self._pend = eng.predict(np.ascontiguousarray(X_pending, dtype=np.float64))  # [T, k]

    def score(self, Xd, alive=None):
        eng = self.engine
        return eng.forest_mc_acq(eng.forest, self.kind, eng._as_dev(Xd), self._counts, self._order, self.S, self._pend, self.best_f,
                                 self.sign, self.beta, alive)

    def greedy(self, Xd, batch_size: int, seed: int, X_pending=None, alive=None) -> GreedyResult:
        eng = self.engine
        torch = eng._torch()
        Xd = eng._as_dev(Xd)
        self.prepare(seed, X_pending)
        alive = torch.ones(Xd.shape[0], dtype=torch.uint8, device=Xd.device) if alive is None else alive.clone()
        indices, values = [], []
        for _ in range(batch_size):
            scores = self.score(Xd, alive)
            val, idx = eng.argmax(scores)
            indices.append(int(idx)), values.append(float(val))
            column = eng.forest_predict(eng.forest, Xd[int(idx):int(idx) + 1])  # [T, 1]
            self._pend = column if self._pend is None else torch.cat([self._pend, column], dim=1).contiguous()
            alive[int(idx)] = 0
        return GreedyResult(indices, values)

    # ---- the recommender's surface (``baybe_amd.scoring``): ONE sampler seed per call (the posterior has no pruning draw) ---------
    supports_continuous = False
    check_request = staticmethod(check_joint_batch)

    def select(self, X, q, *, seeds, X_pending=None, alive=None, shard=None) -> GreedyResult:
        refuse_shard(shard, shard_text(self.name))
        return self.greedy(X, q, seeds(), X_pending, alive)

    def values(self, X, *, seeds, X_pending=None):
        self.prepare(seeds(), X_pending)
        return self.score(self.engine._as_dev(X))

    def joint_value(self, batch, *, seeds, X_pending=None) -> float:
        """Incremental: the value of the batch's last point with the others (and the pending rows) pending."""
        rest = [batch[:-1]] + ([X_pending] if X_pending is not None else [])
        self.prepare(seeds(), np.vstack(rest) if len(batch) > 1 or X_pending is not None else None)
        return float(self.score(self.engine._as_dev(batch[-1:])).cpu().numpy()[0])


# ---- the surrogate -----------------------------------------------------------------------------------------------------------------------
class HipForestSurrogateImpl:
    """Behaviour of the random forest surrogate scored on an MI355X (no fields: ``attrs.make_class`` attaches them, below for the
    stand-alone class and in ``baybe_amd.plugin.make_baybe_forest_surrogate`` on top of BayBE's ``Surrogate``)."""

    __slots__ = ()

    supports_transfer_learning: ClassVar[bool] = False
    supports_multi_output: ClassVar[bool] = False
    is_ensemble: ClassVar[bool] = True
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
        # unchanged context -> no refit, keyed like HipGPSurrogateImpl.fit: the encoding, the target definition, the measurements
        mhash = (
            tuple(searchspace.comp_rep_columns),
            np.asarray(searchspace.scaling_bounds.to_numpy(), dtype=np.float64).tobytes(),
            getattr(searchspace, "task_idx", None),
            n_tasks,
            _objective_key(objective),
            repr(sorted(self.model_params.items(), key=lambda kv: kv[0])),
            _frame_hash(measurements),
        )
        if self._engine is not None and self._engine.packed is not None and mhash == self._measurements_hash:
            self._searchspace, self._objective = searchspace, objective
            return
        if n_tasks > 1:
            raise ValueError(
                f"The search space contains task parameters but the selected "
                f"surrogate model type ({self.__class__.__name__}) does not "
                f"support transfer learning."
            )
        refuse_continuous(searchspace)
        target = quantities[0]
        needs = getattr(objective, "_model_quantities_to_target_names", None)
        names = list(needs[target.name]) if needs is not None else [target.name]
        if any(pd.isna(measurements[nm].to_numpy()).any() for nm in names):
            raise ValueError(f"Missing target values are not supported: {[t.name for t in objective.targets]}")
        comp = searchspace.transform(measurements, allow_extra=True)
        train_x = np.ascontiguousarray(comp.to_numpy(dtype=np.float64))  # the raw comp rep: trees need no input scaling
        train_y = pre_transformed(objective, measurements)[target.name].to_numpy(dtype=np.float64)  # ... and no output scaling
        if np.isnan(train_x).any():
            raise ValueError("NaN among the training rows: the forest surrogate does not route missing values.")
        packed, model = fit_forest(train_x, train_y, self.model_params)
        if self._engine is None:
            self._engine = HipForestEngine(self.device)
        self._engine._X_train, self._engine._y_train = train_x, train_y
        self._engine.set_forest(packed, train_x.shape[1])
        self._model = model
        self._searchspace, self._objective, self._measurements_hash = searchspace, objective, mhash

    def to_botorch(self):
        raise IncompatibilityError(
            "HipRandomForestSurrogate does not wrap a BoTorch model: the ensemble posterior and the acquisition "
            "are evaluated by libbaybe_hip. Use posterior_mean_var() / posterior_stats(), or a "
            "BotorchRecommender with baybe's RandomForestSurrogate for BoTorch-only features."
        )

    # ---- abstract hooks of baybe.surrogates.base.Surrogate (base.py:274-306, 467-469) ------------------------
    def _fit(self, train_x, train_y) -> None:
        raise NotImplementedError("HipRandomForestSurrogate.fit() fits, packs and uploads the forest itself.")

    def _posterior(self, candidates_comp_scaled, /):
        raise IncompatibilityError(
            "HipRandomForestSurrogate builds no BoTorch posterior: the [n_estimators, N] prediction matrix an EnsemblePosterior wraps "
            "is what the device path does without. Use posterior_mean_var() / posterior_stats()."
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
        """(mean over trees, unbiased variance over trees) as device tensors [N]; the variance is identically 0 for one tree."""
        return self.engine.posterior(candidates_comp)

    def posterior_stats(self, candidates: pd.DataFrame, stats=("mean", "std")) -> pd.DataFrame:
        """``Surrogate.posterior_stats`` (surrogates/base.py:308-384): ``<target>_<stat>`` columns; the ensemble posterior has no
        quantile."""
        eng = self.engine
        for s in (x for x in stats if isinstance(x, float)):
            if not 0.0 < s < 1.0:
                raise ValueError(
                    f"Posterior quantile statistics can only be computed for quantiles between 0 and 1 "
                    f"(non-inclusive). Provided value: '{s}' as part of '{stats=}'."
                )
        for s in stats:
            if isinstance(s, float) or s not in ("mean", "std", "var"):
                raise TypeError(
                    f"The utilized posterior of type 'EnsemblePosterior' does not support the "
                    f"statistic associated with the requested input '{s}'."
                )
        comp = self._searchspace.transform(candidates, allow_extra=True)
        mean, var = eng.posterior(np.ascontiguousarray(comp.to_numpy(dtype=np.float64)))
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        name = modeled_quantities(self._objective)[0].name
        out = pd.DataFrame(index=candidates.index)
        for s in stats:
            out[f"{name}_{s}"] = {"mean": mean, "std": np.sqrt(var), "var": var}[s]
        return out


def refuse_continuous(searchspace) -> None:
    """Non-GP models take discrete spaces only (``surrogates/base.py:403-404``)."""
    cont = getattr(searchspace, "continuous", None)
    if cont is not None and not getattr(cont, "is_empty", True):
        raise NotImplementedError(
            "Continuous and hybrid search spaces are not supported by non-GP surrogate models: HipRandomForestSurrogate scores "
            "the rows of a discrete search space."
        )


def is_constant_target(train_y: np.ndarray) -> bool:
    """``catch_constant_targets``: one value, or an (unbiased, ``torch.std``) standard deviation below 1e-6."""
    train_y = np.asarray(train_y, dtype=np.float64)
    return train_y.size == 1 or float(np.std(train_y, ddof=1)) < CONSTANT_TARGET_STD


def fit_forest(train_x: np.ndarray, train_y: np.ndarray, model_params: dict):
    """(packed forest, the scikit-learn model or None): the host-side fit."""
    if is_constant_target(train_y):
        return single_leaf_forest(float(np.mean(train_y))), None
    from sklearn.ensemble import RandomForestRegressor

    model = RandomForestRegressor(**model_params)
    model.fit(train_x, np.asarray(train_y, dtype=np.float64).ravel())
    return pack_forest(model.estimators_), model


def forest_surrogate_fields(with_runtime_state: bool = True) -> dict:
    """attrs fields of the forest surrogate.  ``with_runtime_state=False`` leaves out the fields BayBE's ``Surrogate`` base already
    declares (``surrogates/base.py:93-103``)."""
    f = {
        "model_params": field(factory=dict, converter=dict, validator=validate_model_params),
        "device": field(default=0),  # HIP device ordinal
        "_engine": field(init=False, default=None, eq=False, repr=False),
        "_model": field(init=False, default=None, eq=False, repr=False),  # the fitted RandomForestRegressor (None: constant targets)
    }
    if with_runtime_state:
        for name in ("_searchspace", "_objective", "_measurements_hash"):
            f[name] = field(init=False, default=None, eq=False, repr=False)
    return f


HipRandomForestSurrogate = attrs.make_class("HipRandomForestSurrogate", forest_surrogate_fields(), bases=(HipForestSurrogateImpl,),
                                            slots=True)
HipRandomForestSurrogate.__doc__ = "A random forest surrogate scored on an MI355X (stand-alone class)."
HipRandomForestSurrogate.__module__ = __name__
