"""Declarative acquisition functions of the HIP path (mirror of ``baybe/acquisition/acqfs.py``).

Only what the hot path scores on the device is defined: qLogEI (``acqfs.py:219-223``), the noisy forms qNEI / qLogNEI
(``acqfs.py:226-243``), the noisy Pareto functions qLogNEHVI / qNEHVI (``acqfs.py:467-484``) and qLogNParEGO
(``acqfs.py:328-336``), the non-noisy pair qEHVI / qLogEHVI (``acqfs.py:429-464``; opt-in, ``ehvi="device"``), and the closed-form/posterior read-backs built from (mean, variance).  BoTorch's defaults that BayBE
does not expose are recorded as explicit fields (sample count 512; fat=True, tau_relu=1e-6,
tau_max=1e-2 are compiled into the kernels)."""

from __future__ import annotations

from typing import ClassVar

import attrs
from attrs import define, field
from attrs.converters import optional as optional_c
from attrs.validators import ge, gt, instance_of, le
from attrs.validators import optional as optional_v


@define(frozen=True)
class qLogExpectedImprovement:
    """Logarithmic Monte-Carlo expected improvement (BoTorch qLogExpectedImprovement)."""

    abbreviation: ClassVar[str] = "qLogEI"
    supports_batching: ClassVar[bool] = True
    supports_pending_experiments: ClassVar[bool] = True
    supports_multi_output: ClassVar[bool] = False
    is_mc: ClassVar[bool] = True

    n_mc_samples: int = field(default=512, validator=[instance_of(int), ge(1)])
    """Sobol base samples (BoTorch default for qLogEI; BayBE has no knob for it)."""


    kind: ClassVar[str] = "qLogEI"
    is_analytic: ClassVar[bool] = False


qLogEI = qLogExpectedImprovement


def _mc_class(name: str, abbr: str, doc: str, with_beta: bool = False):
    """Declarative MC acquisition function scored by ``bbh_mc_acq_*`` (acqfs.py:180-290)."""
    ns = {
        "__doc__": doc, "abbreviation": abbr, "kind": abbr, "supports_batching": True, "supports_pending_experiments": True,
        "supports_multi_output": False, "is_mc": True, "is_analytic": False,
        "__annotations__": {"abbreviation": ClassVar[str], "kind": ClassVar[str], "supports_batching": ClassVar[bool],
                            "supports_pending_experiments": ClassVar[bool], "supports_multi_output": ClassVar[bool],
                            "is_mc": ClassVar[bool], "is_analytic": ClassVar[bool], "n_mc_samples": int},
        "n_mc_samples": field(default=512, validator=[instance_of(int), ge(1)]),
    }
    if with_beta:
        ns["__annotations__"]["beta"] = float
        ns["beta"] = field(default=0.2, converter=float)
    return define(frozen=True)(type(name, (), ns))


def _analytic_class(name: str, abbr: str, doc: str, with_beta: bool = False, with_maximize: bool = False):
    """Declarative analytic acquisition function scored by ``bbh_analytic_acq`` (q = 1 only)."""
    ns = {
        "__doc__": doc, "abbreviation": abbr, "kind": abbr, "supports_batching": False, "supports_pending_experiments": False,
        "supports_multi_output": False, "is_mc": False, "is_analytic": True,
        "__annotations__": {"abbreviation": ClassVar[str], "kind": ClassVar[str], "supports_batching": ClassVar[bool],
                            "supports_pending_experiments": ClassVar[bool], "supports_multi_output": ClassVar[bool],
                            "is_mc": ClassVar[bool], "is_analytic": ClassVar[bool]},
    }
    if with_beta:
        ns["__annotations__"]["beta"] = float
        ns["beta"] = field(default=0.2, converter=float)
    if with_maximize:
        ns["__annotations__"]["maximize"] = bool
        ns["maximize"] = field(default=True, validator=instance_of(bool))
    return define(frozen=True)(type(name, (), ns))


qExpectedImprovement = _mc_class("qExpectedImprovement", "qEI", "Monte Carlo based expected improvement.")
qProbabilityOfImprovement = _mc_class("qProbabilityOfImprovement", "qPI", "Monte Carlo based probability of improvement.")
qSimpleRegret = _mc_class("qSimpleRegret", "qSR", "Monte Carlo based simple regret.")
qUpperConfidenceBound = _mc_class("qUpperConfidenceBound", "qUCB", "Monte Carlo based upper confidence bound.", with_beta=True)
qPosteriorStandardDeviation = _mc_class("qPosteriorStandardDeviation", "qPSTD", "Monte Carlo based posterior standard deviation.")
PosteriorMean = _analytic_class("PosteriorMean", "PM", "Posterior mean.")
PosteriorStandardDeviation = _analytic_class("PosteriorStandardDeviation", "PSTD", "Posterior standard deviation.", with_maximize=True)
UpperConfidenceBound = _analytic_class("UpperConfidenceBound", "UCB", "Analytical upper confidence bound.", with_beta=True)
ExpectedImprovement = _analytic_class("ExpectedImprovement", "EI", "Analytical expected improvement.")
LogExpectedImprovement = _analytic_class("LogExpectedImprovement", "LogEI", "Logarithmic analytical expected improvement.")
ProbabilityOfImprovement = _analytic_class("ProbabilityOfImprovement", "PI", "Analytical probability of improvement.")
qEI, qPI, qSR, qUCB, qPSTD = (qExpectedImprovement, qProbabilityOfImprovement, qSimpleRegret, qUpperConfidenceBound,
                              qPosteriorStandardDeviation)
PM, PSTD, UCB, EI, LogEI, PI = (PosteriorMean, PosteriorStandardDeviation, UpperConfidenceBound, ExpectedImprovement,
                                LogExpectedImprovement, ProbabilityOfImprovement)
_SINGLE_OUTPUT = {c.abbreviation: c for c in (qExpectedImprovement, qProbabilityOfImprovement, qSimpleRegret,
                                               qUpperConfidenceBound, qPosteriorStandardDeviation, PosteriorMean,
                                               PosteriorStandardDeviation, UpperConfidenceBound, ExpectedImprovement,
                                               LogExpectedImprovement, ProbabilityOfImprovement)}


def _convert_ref(value):
    if value is None or isinstance(value, float):
        return value
    if isinstance(value, int):
        return float(value)
    return tuple(float(v) for v in value)


@define(frozen=True)
class qLogNoisyExpectedHypervolumeImprovement:
    """Logarithmic Monte-Carlo noisy expected hypervolume improvement (``acqfs.py:477-484``)."""

    abbreviation: ClassVar[str] = "qLogNEHVI"
    kind: ClassVar[str] = "qLogNEHVI"
    supports_batching: ClassVar[bool] = True
    supports_pending_experiments: ClassVar[bool] = True
    supports_multi_output: ClassVar[bool] = True
    is_mc: ClassVar[bool] = True

    reference_point = field(default=None, converter=_convert_ref)
    """None: computed from the measured targets; float: the factor of ``compute_ref_point``;
    iterable: the coordinates themselves (``acqfs.py:337-347``)."""

    prune_baseline: bool = field(default=True, validator=instance_of(bool))
    """Auto-prune baseline points that are unlikely to be Pareto-optimal."""

    n_mc_samples: int = field(default=128, validator=[instance_of(int), ge(1)])
    """Sobol base samples (BoTorch default for multi-objective MC acquisition functions)."""


qLogNEHVI = qLogNoisyExpectedHypervolumeImprovement


@define(frozen=True)
class qNoisyExpectedHypervolumeImprovement:
    """Monte-Carlo noisy expected hypervolume improvement (``acqfs.py:467-474``), scored by ``baybe_amd.nehvi.HipNEHVIPlain``."""

    abbreviation: ClassVar[str] = "qNEHVI"
    kind: ClassVar[str] = "qNEHVI"
    supports_batching: ClassVar[bool] = True
    supports_pending_experiments: ClassVar[bool] = True
    supports_multi_output: ClassVar[bool] = True
    is_mc: ClassVar[bool] = True
    is_analytic: ClassVar[bool] = False

    reference_point = field(default=None, converter=_convert_ref)
    """As for qLogNEHVI."""

    prune_baseline: bool = field(default=True, validator=instance_of(bool))
    """Auto-prune baseline points that are unlikely to be Pareto-optimal."""

    n_mc_samples: int = field(default=128, validator=[instance_of(int), ge(1)])
    """Sobol base samples (BoTorch default for multi-objective MC acquisition functions)."""


qNEHVI = qNoisyExpectedHypervolumeImprovement


def _convert_alpha(value):
    return None if value is None else float(value)


def _ehvi_class(name: str, abbr: str, doc: str):
    """Declarative (non-noisy) expected hypervolume improvement (``acqfs.py:429-464``), scored by ``baybe_amd.ehvi.HipEHVI`` under
    the recommender's ``ehvi="device"``.  There is no ``prune_baseline``: nothing is sampled at the measurement rows."""
    ns = {
        "__doc__": doc, "abbreviation": abbr, "kind": abbr, "supports_batching": True, "supports_pending_experiments": True,
        "supports_multi_output": True, "is_mc": True, "is_analytic": False,
        "__annotations__": {"abbreviation": ClassVar[str], "kind": ClassVar[str], "supports_batching": ClassVar[bool],
                            "supports_pending_experiments": ClassVar[bool], "supports_multi_output": ClassVar[bool],
                            "is_mc": ClassVar[bool], "is_analytic": ClassVar[bool], "n_mc_samples": int},
        # None: computed from the measured targets; float: the factor of ``compute_ref_point``; iterable: the coordinates
        "reference_point": field(default=None, converter=_convert_ref),
        # threshold of the partitioning: None (BoTorch's default, 0 for up to 4 objectives) and 0 are the exact partitioning; a positive
        # value asks for the approximate one, which the recommender refuses
        "alpha": field(default=None, converter=_convert_alpha),
        # Sobol base samples (BoTorch default for multi-objective MC acquisition functions)
        "n_mc_samples": field(default=128, validator=[instance_of(int), ge(1)]),
    }
    return define(frozen=True)(type(name, (), ns))


qExpectedHypervolumeImprovement = _ehvi_class("qExpectedHypervolumeImprovement", "qEHVI",
                                              "Monte Carlo based expected hypervolume improvement.")
qLogExpectedHypervolumeImprovement = _ehvi_class("qLogExpectedHypervolumeImprovement", "qLogEHVI",
                                                 "Logarithmic Monte Carlo based expected hypervolume improvement.")
qEHVI, qLogEHVI = qExpectedHypervolumeImprovement, qLogExpectedHypervolumeImprovement
_EHVI = {c.abbreviation: c for c in (qExpectedHypervolumeImprovement, qLogExpectedHypervolumeImprovement)}


def _convert_weights(value):
    return None if value is None else tuple(float(v) for v in value)


@define(frozen=True)
class qLogNParEGO:
    """Pareto optimization via Chebyshev scalarization of the targets (``acqfs.py:328-336``), scored by
    ``baybe_amd.nparego.HipNParEGO``."""

    abbreviation: ClassVar[str] = "qLogNParEGO"
    kind: ClassVar[str] = "qLogNParEGO"
    supports_batching: ClassVar[bool] = True
    supports_pending_experiments: ClassVar[bool] = True
    supports_multi_output: ClassVar[bool] = True
    is_mc: ClassVar[bool] = True
    is_analytic: ClassVar[bool] = False

    prune_baseline: bool = field(default=True, validator=instance_of(bool))
    """Auto-prune baseline points that are unlikely to be the best of any joint posterior sample."""

    n_mc_samples: int = field(default=512, validator=[instance_of(int), ge(1)])
    """Sobol base samples (the single-output MC default that reaches qLogNEI's constructor; BayBE has no knob for it)."""

    scalarization_weights = field(default=None, converter=_convert_weights)
    """Weights on the simplex, one per target (BoTorch's argument of that name; BayBE has no knob for it).  None: drawn from
    torch's global generator when the acquisition function is built (``sample_simplex``)."""

    @scalarization_weights.validator
    def _check_weights(self, _, value):
        if value is not None and (any(not 0.0 <= v <= 1.0 for v in value) or abs(sum(value) - 1.0) > 1e-9):
            raise ValueError(f"scalarization_weights must be non-negative and sum to 1, got {value!r}")


_NOISY_PARETO = {c.abbreviation: c for c in (qLogNoisyExpectedHypervolumeImprovement, qNoisyExpectedHypervolumeImprovement, qLogNParEGO)}


def _nei_class(name: str, abbr: str, doc: str):
    """Declarative noisy expected improvement (``acqfs.py:226-243``), scored by ``baybe_amd.nei.HipNEI``."""
    ns = {
        "__doc__": doc, "abbreviation": abbr, "kind": abbr, "supports_batching": True, "supports_pending_experiments": True,
        "supports_multi_output": False, "is_mc": True, "is_analytic": False,
        "__annotations__": {"abbreviation": ClassVar[str], "kind": ClassVar[str], "supports_batching": ClassVar[bool],
                            "supports_pending_experiments": ClassVar[bool], "supports_multi_output": ClassVar[bool],
                            "is_mc": ClassVar[bool], "is_analytic": ClassVar[bool], "prune_baseline": bool, "n_mc_samples": int},
        # Auto-prune baseline points that are unlikely to be the best of any joint posterior sample (prune_inferior_points).
        "prune_baseline": field(default=True, validator=instance_of(bool)),
        # Sobol base samples (BoTorch default for single-output MC acquisition functions; BayBE has no knob for it).
        "n_mc_samples": field(default=512, validator=[instance_of(int), ge(1)]),
    }
    return define(frozen=True)(type(name, (), ns))


qNoisyExpectedImprovement = _nei_class("qNoisyExpectedImprovement", "qNEI", "Monte Carlo based noisy expected improvement.")
qLogNoisyExpectedImprovement = _nei_class("qLogNoisyExpectedImprovement", "qLogNEI",
                                          "Logarithmic Monte Carlo based noisy expected improvement.")
qNEI, qLogNEI = qNoisyExpectedImprovement, qLogNoisyExpectedImprovement
_NOISY_EI = {c.abbreviation: c for c in (qNoisyExpectedImprovement, qLogNoisyExpectedImprovement)}


def _convert_sampling_method(value) -> str:
    """``DiscreteSamplingMethod`` (utils/sampling_algorithms.py:175-182) by value or member, kept as its value."""
    name = str(getattr(value, "value", value))
    if name not in ("Random", "FPS"):
        raise ValueError(f"'{value}' is not a valid DiscreteSamplingMethod")
    return name


@define(frozen=True)
class qNegIntegratedPosteriorVariance:
    """Monte Carlo based negative integrated posterior variance (``acqfs.py:29-138``): the reference's acquisition function for
    active learning.  Scored by ``baybe_amd.nipv.HipNIPV`` under the recommender's ``nipv="device"``; no samples are drawn - the
    value is a closed form of the posterior covariance with the integration points (``csrc/bbh_nipv.hip``)."""

    abbreviation: ClassVar[str] = "qNIPV"
    kind: ClassVar[str] = "qNIPV"
    supports_batching: ClassVar[bool] = True
    supports_pending_experiments: ClassVar[bool] = True
    supports_multi_output: ClassVar[bool] = False
    is_mc: ClassVar[bool] = True
    is_analytic: ClassVar[bool] = False

    sampling_n_points: int | None = field(validator=optional_v([instance_of(int), gt(0)]), default=None)
    """Number of data points sampled for integrating the posterior.  Cannot be used if ``sampling_fraction`` is not None."""

    sampling_fraction: float | None = field(converter=optional_c(float), validator=optional_v([gt(0.0), le(1.0)]))
    """Fraction of data sampled for integrating the posterior.  Cannot be used if ``sampling_n_points`` is not None."""

    sampling_method: str = field(converter=_convert_sampling_method, default="Random")
    """Sampling strategy used for integrating the posterior ("Random" or "FPS")."""

    @sampling_fraction.default
    def _default_sampling_fraction(self):
        """If no sampling quantities are provided, use all points by default."""
        return 1.0 if self.sampling_n_points is None else None

    @sampling_fraction.validator
    def _validate_sampling_fraction(self, attr, value) -> None:
        """If both sampling quantities are specified, raise an error."""
        if None not in (self.sampling_fraction, self.sampling_n_points):
            raise ValueError(
                f"For '{self.__class__.__name__}', the attributes '{attr.name}' and "
                f"'{attrs.fields(self.__class__).sampling_n_points.name}' cannot "
                f"be specified at the same time."
            )


qNIPV = qNegIntegratedPosteriorVariance


def convert_acqf(acqf, ehvi: str = "refuse", nipv: str = "refuse"):
    """``baybe.acquisition.utils.convert_acqf``: accept abbreviations / BayBE objects.  ``ehvi``: the recommender's setting of that
    name - "device" converts qEHVI / qLogEHVI (abbreviations, full names, our instances, the reference's objects by class name),
    "refuse" refuses them and names the setting.  ``nipv``: the same for qNIPV (``baybe_amd.nipv``)."""
    name = acqf if isinstance(acqf, str) else type(acqf).__name__
    if name in ("qNIPV", "qNegIntegratedPosteriorVariance"):
        if nipv != "device":
            from baybe_amd.exceptions import IncompatibleAcquisitionFunctionError

            raise IncompatibleAcquisitionFunctionError(
                f"The HIP recommender scores the MC / analytic EI-PI-UCB-SR families, qNEI / qLogNEI, qLogNEHVI / qNEHVI and "
                f"qLogNParEGO on the device; '{name}' is not available on this path. Pass nipv='device' to the recommender to "
                f"score qNIPV on the device over discrete search spaces."
            )
        if isinstance(acqf, qNegIntegratedPosteriorVariance):
            return acqf
        if isinstance(acqf, str):
            return qNegIntegratedPosteriorVariance()
        return qNegIntegratedPosteriorVariance(sampling_n_points=getattr(acqf, "sampling_n_points", None),
                                               sampling_fraction=getattr(acqf, "sampling_fraction", None),
                                               sampling_method=getattr(acqf, "sampling_method", "Random"))
    for abbr, cls in _EHVI.items():
        if name in (abbr, cls.__name__):
            if ehvi != "device":
                from baybe_amd.exceptions import IncompatibleAcquisitionFunctionError

                raise IncompatibleAcquisitionFunctionError(
                    f"The HIP recommender scores the MC / analytic EI-PI-UCB-SR families, qNEI / qLogNEI, qLogNEHVI / qNEHVI and "
                    f"qLogNParEGO on the device; '{name}' is not available on this path. Pass ehvi='device' to the recommender to "
                    f"score qEHVI / qLogEHVI on the device by joint q-batch inclusion-exclusion."
                )
            if isinstance(acqf, cls):
                return acqf
            if isinstance(acqf, str):
                return cls()
            return cls(reference_point=getattr(acqf, "reference_point", None), alpha=getattr(acqf, "alpha", None))
    if acqf is None or isinstance(acqf, (qLogExpectedImprovement, *_NOISY_PARETO.values())):
        return acqf
    if type(acqf) in _SINGLE_OUTPUT.values() or type(acqf) in _NOISY_EI.values():
        return acqf
    name = acqf if isinstance(acqf, str) else type(acqf).__name__
    for abbr, cls in _NOISY_EI.items():
        if name in (abbr, cls.__name__):
            return cls() if isinstance(acqf, str) else cls(prune_baseline=getattr(acqf, "prune_baseline", True))
    for abbr, cls in _SINGLE_OUTPUT.items():
        if name in (abbr, cls.__name__):
            kw = {}
            for attr in ("beta", "maximize"):
                if not isinstance(acqf, str) and hasattr(acqf, attr) and attr in {a.name for a in cls.__attrs_attrs__}:
                    kw[attr] = getattr(acqf, attr)
            return cls(**kw)
    if name in ("qLogEI", "qLogExpectedImprovement"):
        return qLogExpectedImprovement()
    for abbr, cls in _NOISY_PARETO.items():
        if name in (abbr, cls.__name__):
            kw = {}
            if not isinstance(acqf, str):
                kw = {"prune_baseline": getattr(acqf, "prune_baseline", True)}
                if abbr != "qLogNParEGO":
                    kw["reference_point"] = getattr(acqf, "reference_point", None)
            return cls(**kw)
    from baybe_amd.exceptions import IncompatibleAcquisitionFunctionError

    raise IncompatibleAcquisitionFunctionError(
        f"The HIP recommender scores the MC / analytic EI-PI-UCB-SR families, qNEI / qLogNEI, qLogNEHVI / qNEHVI and qLogNParEGO on the device; '{name}' is not available on this path."
    )
