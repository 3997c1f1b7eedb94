"""Exact Shapley explanations of a fitted surrogate, computed on the device: the counterpart of ``baybe.insights.SHAPInsight``
(``baybe/insights/shap.py``) for the surrogates of this package.

Definition.  The features are M groups of comp-rep columns: in the experimental representation one group is one parameter (a
one-hot or substance parameter owns several columns), with ``use_comp_rep=True`` every comp-rep column is its own group.  For an
explained row ``x_r`` and the background rows ``b_1 .. b_B`` the value of a coalition S is

    v(r, S) = (1 / B) sum_b f(compose(x_r on the groups of S, b elsewhere))

with f the surrogate's posterior mean in the target's original scale (the scale ``posterior_stats`` reports), the Shapley value is

    phi_g(r) = sum over S in G \\ {g} of |S|! (M - |S| - 1)! / M! * [v(r, S + g) - v(r, S)]

i.e. ``phi[r, :] = W v[r, :]`` with the fixed ``[M, 2^M]`` matrix W of ``shapley_matrix``, and ``base_value = v(., {}) =
mean_b f(b)``.  These are the exact interventional Shapley values of the model's mean with the given background: what the
reference's default ``shap.KernelExplainer`` returns whenever its budget enumerates every coalition (M <= 11 with the default
``nsamples``), and what it approximates by sampling above that.  Every coalition is visited, so M stops at 16.

``HipGP.shap_values`` evaluates this in two forms (``include/baybe_hip.h``): ``"fused"`` - per-group partial distances and one
kernel value per (row, coalition, background row, training point), no composed row is ever built - for one stationary kernel, one
task and n <= 512; ``"composed"`` - composed rows through the engine's own ``posterior`` - for every other model (composite / RQ /
periodic kernels, task parameters, n > 512, the forest and the linear surrogate).  ``"auto"`` takes the fused form where it applies.
"""

from __future__ import annotations

import math
from typing import Any

import attrs
import numpy as np
import pandas as pd

from baybe_amd.exceptions import IncompatibilityError, IncompatibleExplainerError, NoMeasurementsError

MAX_FEATURES = 16
EXPLAINERS = ("KernelExplainer", "ExactExplainer")
"""Names ``explainer_cls`` accepts; both mean the exact values here."""
_DEFAULT_EXPLAINER_CLS = "KernelExplainer"


# ---- the weights --------------------------------------------------------------------------------------------------------------------
def shapley_weights(M: int) -> np.ndarray:
    """``w[s] = s! (M - s - 1)! / M!`` for s = 0 .. M - 1: the weight of a coalition of size s that does not hold the feature.
    Integer factorials, one correctly rounded division each (numerator and denominator are below 2^53 for M <= 16)."""
    M = int(M)
    if M < 1:
        raise ValueError("at least one feature")
    return np.array([math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M) for s in range(M)], dtype=np.float64)


def shapley_matrix(M: int) -> np.ndarray:
    """W ``[M, 2^M]`` with ``phi = W v``: ``W[g, S] = w[|S| - 1]`` where bit g of S is set, ``-w[|S|]`` where it is not."""
    w = shapley_weights(M)
    S = np.arange(1 << M, dtype=np.int64)
    size = np.zeros(1 << M, dtype=np.int64)
    for g in range(M):
        size += (S >> g) & 1
    W = np.empty((M, 1 << M), dtype=np.float64)
    for g in range(M):
        has = ((S >> g) & 1).astype(bool)
        W[g, has] = w[size[has] - 1]
        W[g, ~has] = -w[size[~has]]
    return W


def _refuse_too_many(M: int) -> None:
    if M > MAX_FEATURES:
        raise IncompatibilityError(
            f"The exact enumeration of coalitions stops at {MAX_FEATURES} features and {M} were requested (2^M coalitions per "
            f"explained row). Explain the experimental representation (use_comp_rep=False), where a parameter is one feature, or "
            f"a search space with fewer parameters."
        )


# ---- features -----------------------------------------------------------------------------------------------------------------------
def feature_groups(searchspace, use_comp_rep: bool = False):
    """``(groups [d] int32, names)``: the feature each comp-rep column belongs to (-1: none) and the features' names, in group
    order.  Experimental representation: one feature per parameter, its columns from ``get_comp_rep_parameter_indices`` where the
    search space has it, else the columns named like the parameter or prefixed ``<name>_``."""
    cols = [str(c) for c in searchspace.comp_rep_columns]
    if use_comp_rep:
        return np.arange(len(cols), dtype=np.int32), cols
    groups = np.full(len(cols), -1, dtype=np.int32)
    names = []
    for p in searchspace.parameters:
        nm = p.name
        if hasattr(searchspace, "get_comp_rep_parameter_indices"):
            hit = [int(i) for i in searchspace.get_comp_rep_parameter_indices(nm)]
        else:
            hit = [i for i, c in enumerate(cols) if c == nm or c.startswith(f"{nm}_")]
        if not hit:
            raise ValueError(f"Parameter '{nm}' owns no column of the computational representation.")
        groups[hit] = len(names)
        names.append(nm)
    return groups, names


def _engine_of(surrogate):
    eng = getattr(surrogate, "engine", None)  # (raises ModelNotTrainedError before training)
    if eng is None or not hasattr(eng, "shap_values"):
        raise IncompatibilityError(f"'{type(surrogate).__name__}' has no device engine to explain.")
    if getattr(eng, "_comm", None) is not None:
        raise IncompatibilityError("Shapley explanations do not run over row shards: explain on a single-device engine.")
    return eng


def _comp_rows(searchspace, df: pd.DataFrame, use_comp_rep: bool) -> np.ndarray:
    if use_comp_rep:
        comp = df[[c for c in searchspace.comp_rep_columns]]
    else:
        comp = searchspace.transform(df, allow_extra=True)
        comp = comp[[c for c in searchspace.comp_rep_columns]]
    return np.ascontiguousarray(comp.to_numpy(dtype=np.float64))


def shapley_values(surrogate, data: pd.DataFrame, background: pd.DataFrame, use_comp_rep: bool = False, form: str = "auto"):
    """``(phi [R, M], base_value, feature_names)`` of a fitted single-output surrogate: the rows of ``data`` explained against
    ``background``.  Both frames hold the parameters' columns (``use_comp_rep=False``; extra columns are ignored) or the comp-rep
    columns (``use_comp_rep=True``).  The features come in the order of ``feature_names``: the search space's parameters, or its
    comp-rep columns."""
    searchspace = surrogate._searchspace
    eng = _engine_of(surrogate)
    groups, names = feature_groups(searchspace, use_comp_rep)
    _refuse_too_many(len(names))
    if len(background) == 0:
        raise ValueError("The provided background data set is empty.")
    X = _comp_rows(searchspace, data, use_comp_rep)
    if len(X) == 0:
        return np.zeros((0, len(names))), float("nan"), names
    Bg = _comp_rows(searchspace, background, use_comp_rep)
    phi, base, _ = eng.shap_values(X, Bg, groups, form=form, n_groups=len(names))
    return phi.cpu().numpy(), float(base), names


# ---- the insight --------------------------------------------------------------------------------------------------------------------
@attrs.frozen(eq=False)
class Explanation:
    """What ``shap.Explanation`` carries of a result: ``values`` [R, M], ``base_values`` [R], ``data`` [R, M] (the explained rows'
    entries, as objects where a parameter is categorical) and ``feature_names``."""

    values: np.ndarray
    base_values: np.ndarray
    data: np.ndarray
    feature_names: list

    @property
    def shape(self):
        return self.values.shape

    def to_shap(self):
        """The same as a ``shap.Explanation`` (needs the ``shap`` package)."""
        shap = _import_shap("Explanation.to_shap")
        return shap.Explanation(values=self.values, base_values=self.base_values, data=self.data, feature_names=self.feature_names)


def _import_shap(who: str):
    try:
        import shap  # type: ignore
    except Exception as ex:  # noqa: BLE001
        raise ImportError(f"'{who}' needs the optional package 'shap', which is not installed. The explanation itself "
                          f"(HipSHAPInsight.explain) does not.") from ex
    return shap


def _single_output_surrogates(cls, surrogate) -> tuple:
    from baybe_amd.surrogates import HipCompositeImpl

    if isinstance(surrogate, HipCompositeImpl):
        return tuple(surrogate.models)
    if hasattr(surrogate, "engine") and hasattr(surrogate, "posterior_stats"):
        return (surrogate,)
    raise ValueError(f"'{cls.__name__}.from_surrogate' only accepts the surrogate models of this package or their "
                     f"'.replicate()'d composites.")


@attrs.define
class HipSHAPInsight:
    """Shapley feature importances of the surrogates of this package (``baybe.insights.SHAPInsight``'s surface)."""

    surrogates: tuple = attrs.field(converter=tuple)
    """One single-output surrogate per target."""

    background_data: pd.DataFrame = attrs.field(validator=attrs.validators.instance_of(pd.DataFrame))
    """The background data set."""

    use_comp_rep: bool = attrs.field(default=False, kw_only=True)
    form: str = attrs.field(default="auto", kw_only=True)
    """``HipGP.shap_values``'s form: ``"auto"``, ``"fused"`` or ``"composed"``."""

    @classmethod
    def from_surrogate(cls, surrogate, data: pd.DataFrame, explainer_cls: Any = _DEFAULT_EXPLAINER_CLS, *, use_comp_rep: bool = False,
                       form: str = "auto") -> "HipSHAPInsight":
        """An insight for a fitted surrogate; ``data`` is the background data set."""
        singles = _single_output_surrogates(cls, surrogate)
        if data.empty:
            raise ValueError("The provided background data set is empty.")
        name = explainer_cls if isinstance(explainer_cls, str) else getattr(explainer_cls, "__name__", repr(explainer_cls))
        if name not in EXPLAINERS:
            raise IncompatibleExplainerError(
                f"The explainer '{name}' is not available on the device: the supported names are '{EXPLAINERS[0]}' and "
                f"'{EXPLAINERS[1]}', which both yield the exact Shapley values here."
            )
        for s in singles:
            _engine_of(s)
            _refuse_too_many(len(feature_groups(s._searchspace, use_comp_rep)[1]))
        return cls(singles, data, use_comp_rep=use_comp_rep, form=form)

    @classmethod
    def from_campaign(cls, campaign, explainer_cls: Any = _DEFAULT_EXPLAINER_CLS, *, use_comp_rep: bool = False,
                      form: str = "auto") -> "HipSHAPInsight":
        """An insight for a campaign's surrogate, with the campaign's measurements as the background."""
        if campaign.measurements.empty:
            raise NoMeasurementsError("The campaign does not contain any measurements.")
        data = campaign.measurements[[p.name for p in campaign.parameters]]
        background = campaign.searchspace.transform(data) if use_comp_rep else data
        return cls.from_surrogate(campaign.get_surrogate(), background, explainer_cls=explainer_cls, use_comp_rep=use_comp_rep, form=form)

    @classmethod
    def from_recommender(cls, recommender, searchspace, objective, measurements: pd.DataFrame,
                         explainer_cls: Any = _DEFAULT_EXPLAINER_CLS, *, use_comp_rep: bool = False,
                         form: str = "auto") -> "HipSHAPInsight":
        """An insight for a recommender's surrogate, trained on ``measurements``, which are the background as well."""
        if not hasattr(recommender, "get_surrogate"):
            raise TypeError(
                f"The provided recommender does not provide a surrogate model. "
                f"'{cls.__name__}' needs a surrogate model and thus only works with "
                f"model-based recommenders."
            )
        surrogate = recommender.get_surrogate(searchspace, objective, measurements)
        data = measurements[[p.name for p in searchspace.parameters]]
        return cls.from_surrogate(surrogate, searchspace.transform(data) if use_comp_rep else data, explainer_cls=explainer_cls,
                                  use_comp_rep=use_comp_rep, form=form)

    def explain_target(self, target_index: int, data: pd.DataFrame | None = None, /) -> Explanation:
        """The explanation of ``data`` (default: the background) for one target.  Extra columns are ignored; the output's features
        come in the order of ``data``'s columns."""
        bg = self.background_data
        if data is None:
            data = bg
        elif not set(bg.columns).issubset(data.columns):
            raise ValueError("The provided dataframe must contain all columns that were used for the background data.")
        aligned = data[bg.columns]
        phi, base, names = shapley_values(self.surrogates[target_index], aligned, bg, use_comp_rep=self.use_comp_rep, form=self.form)
        missing = [nm for nm in names if nm not in bg.columns]
        if missing:
            raise ValueError(f"The background data set lacks the columns {missing} of the explained representation.")
        # features in the order of the caller's columns (those the background knows)
        order = [names.index(c) for c in data.columns if c in names]
        feats = [names[i] for i in order]
        return Explanation(np.ascontiguousarray(phi[:, order]), np.full(len(aligned), base), aligned[feats].to_numpy(), feats)

    def explain(self, data: pd.DataFrame | None = None, /) -> tuple:
        """The explanations of ``data`` for all targets."""
        return tuple(self.explain_target(k, data) for k in range(len(self.surrogates)))

    def plot(self, plot_type: str, data: pd.DataFrame | None = None, /, **kwargs):
        """Plots are drawn by the ``shap`` package: with it installed, pass ``explain_target(...).to_shap()`` to ``shap.plots``."""
        _import_shap("HipSHAPInsight.plot")
        raise NotImplementedError("HipSHAPInsight draws no plots itself: pass explain_target(...).to_shap() to shap.plots.")
