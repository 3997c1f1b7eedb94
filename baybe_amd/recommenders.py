"""Host-side mirror of ``BotorchRecommender`` for purely discrete search spaces, on the HIP path.

Same call structure as the reference:
``recommend`` (``pure/bayesian/base.py:130-197``) -> fit the surrogate and set up the acquisition
(``_setup_botorch_acqf``, ``base.py:87-111``; best_f / X_pending semantics of
``acquisition/_builder.py:195-334``) -> ``_recommend_with_discrete_parts``
(``pure/base.py:248-310``) -> ``_recommend_discrete`` (``botorch/core.py:155-184``) ->
``recommend_discrete_without_subsets`` (``botorch/discrete.py:78-142``), whose
``optimize_acqf_discrete`` call is replaced by ``HipGP.greedy_qlogei``.

Differences that are deliberate: the comp-rep rows of the
candidates are taken positionally from ``subspace_discrete.comp_rep`` (no re-encoding of N rows,
no float-key merge), so exactly ``batch_size`` index labels are returned even if the search
space contains duplicate rows.
"""

from __future__ import annotations

from typing import ClassVar

import attrs
import numpy as np
import pandas as pd
from attrs import field
from attrs.validators import ge, gt, instance_of

from baybe_amd import _lib
from baybe_amd.acquisition import convert_acqf, qLogExpectedImprovement, qLogNoisyExpectedHypervolumeImprovement
from baybe_amd.engine import draw_sampler_seed, sobol_normal_base_samples
from baybe_amd.exceptions import (
    IncompatibilityError,
    IncompatibleAcquisitionFunctionError,
    NotEnoughPointsLeftError,
)
from baybe_amd.surrogates import HipCompositeImpl, HipGaussianProcessSurrogate, _availability_property


MAX_HYBRID_CONTINUOUS = 4  # continuous parameters of a hybrid / continuous space the derivative-free search is validated for
MAX_GRADIENT_CONTINUOUS = 32  # ... and the gradient-based refinement takes (the differentiated columns of one bbh_posterior_grad call)
MAX_GRADIENT_TRAINING_POINTS = 512  # training points of a model bbh_posterior_grad differentiates
MAX_GRADIENT_STARTS = 16384  # starts one gradient refinement advances together
GRADIENT_KERNELS = ("matern32", "matern52", "rbf")


def _hash_buffers(bufs) -> int:
    """64-bit content key of a list of byte buffers: the library's host-side multiply-fold hash over 4 MB pieces on native threads
    (``bbh_content_key``).  python-xxhash keeps the GIL, so the "8 threads" of round 4 hashed the 160 MB comp rep of a 1e6 x 20 grid
    at one core's rate - 5 ms of every ``recommend()``; natively it is memory-bound."""
    import ctypes as C
    import os

    from baybe_amd import _lib

    lib = _lib.load_library()
    n = len(bufs)
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in bufs]
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (C.c_int64 * n)(*[a.size for a in arrs])
    total = sum(a.size for a in arrs)
    threads = 1 if total < (1 << 22) else max(1, min(32, os.cpu_count() or 1))
    return int(lib.bbh_content_key(ptrs, lens, n, threads))


def _content_hash(arr: np.ndarray):
    """Content hash of a numeric array: xxh3 over its buffer (the transposed view if that is the contiguous one - a
    single-dtype DataFrame hands out its block that way - so nothing is copied), large buffers in pieces on a thread
    pool (xxhash releases the GIL)."""
    arr = np.asarray(arr)
    if arr.size == 0:
        return hash((arr.shape, str(arr.dtype)))
    if arr.dtype == object:
        return hash((arr.shape, tuple(arr.ravel().tolist())))
    if not arr.flags.c_contiguous:
        arr = arr.T if arr.T.flags.c_contiguous else np.ascontiguousarray(arr)
    return _hash_buffers([memoryview(arr).cast("B")])


def _frame_content_hash(df: pd.DataFrame):
    """Content hash of a DataFrame's values without materialising them as one array: every column's buffer in pieces on the
    thread pool; columns that are not plain numeric arrays go through ``_content_hash``.  Equal keys
    mean equal content up to the collision chance of a 64-bit hash (2^-64 per pair of contents); the same content in another memory layout (a row-major block against a column-major copy) may key
    differently, which costs one re-upload and nothing else."""
    if df.shape[1] == 0 or not df.iloc[:, 0].to_numpy().flags.c_contiguous:
        return _content_hash(df.to_numpy())  # one 2-D block: ``to_numpy`` is a view, its columns are strided
    cols = [df.iloc[:, j].to_numpy() for j in range(df.shape[1])]
    plain = [a for a in cols if a.dtype != object and a.flags.c_contiguous]
    other = [a for a in cols if not (a.dtype != object and a.flags.c_contiguous)]
    return hash((_hash_buffers([memoryview(a).cast("B") for a in plain]), tuple(_content_hash(a) for a in other),
                 tuple(a.dtype != object and a.flags.c_contiguous for a in cols)))


def _is_multi_output(objective) -> bool:
    """``Objective.is_multi_output`` (objectives/base.py): False for single-target AND desirability objectives."""
    flag = getattr(objective, "is_multi_output", None)
    return bool(flag) if flag is not None else len(objective.targets) > 1


def _check_objective(objective, acqf, desirability: str = "refuse"):
    """What of ``baybe.objectives`` is on the device path, checked before anything is fitted: single targets, with their
    transformation as an objective program (``baybe_amd.objective``), and Pareto stacking of identity / negated targets (SURVEY.md
    §8a row a9).  A ``DesirabilityObjective`` is single-output in the reference (scalarised, optimised with qLogEI,
    ``objectives/desirability.py:222-265``) - treating it as Pareto because it has several targets would answer a different
    question.  Returns the single target's ``ObjectiveProgram`` (None: identity, on the kernels' ``sign`` path) - or, for a
    desirability objective with one model per target under ``desirability="device"``, its ``DesirabilityProgram``."""
    kind = type(objective).__name__
    from baybe_amd.objective import objective_program
    from baybe_amd.surrogates import _target_sign, modeled_quantities

    quantities = modeled_quantities(objective)
    if len(quantities) > 1 and not _is_multi_output(objective):
        # one model per target + a per-sample scalarisation objective (objectives/desirability.py:229-265)
        if desirability != "device":
            raise IncompatibilityError(
                f"Objectives of type '{kind}' scalarise several modeled targets per posterior sample; the HIP path supports "
                f"single-target and Pareto objectives and 'DesirabilityObjective(as_pre_transformation=True)', which scalarises the "
                f"measurements before fitting. Use BotorchRecommender otherwise, or pass desirability='device' to the recommender "
                f"to score the per-sample scalarisation on the device."
            )
        return _check_desirability(objective, acqf)
    if _is_multi_output(objective) and not acqf.supports_multi_output:
        raise IncompatibleAcquisitionFunctionError(
            f"You attempted to use a single-output acquisition function in a "
            f"{len(quantities)}-target multi-output context."
        )
    if not _is_multi_output(objective) and acqf.supports_multi_output:
        raise IncompatibleAcquisitionFunctionError(
            f"The acquisition function '{type(acqf).__name__}' needs a multi-output objective, but a single-target "
            f"objective was given."
        )
    if _is_multi_output(objective) or getattr(acqf, "kind", None) in ("qNEI", "qLogNEI"):
        for target in quantities:  # identity transformations (+ minimisation) only: raises IncompatibilityError
            _target_sign(target)
        return None
    program = objective_program(quantities[0])  # raises IncompatibilityError for what the kernels do not evaluate
    if program is not None and getattr(acqf, "is_analytic", False) and program.as_affine() is None:
        # only an affine map keeps the posterior Gaussian (posterior transform, objectives/single.py:77-91; _builder.py:224-234)
        raise IncompatibilityError(
            f"The selected analytical acquisition function '{type(acqf).__name__}' is incompatible with the assigned objective "
            f"'{kind}' because the former requires a Gaussian distribution and the latter is configured to produce "
            f"non-Gaussian outcomes."
        )
    return program


def _check_desirability(objective, acqf):
    """The ``DesirabilityProgram`` of a desirability objective with one model per target, or why the acquisition function does not
    take it - before anything is fitted."""
    from baybe_amd.desirability import desirability_program

    kind = type(objective).__name__
    program = desirability_program(objective)  # raises IncompatibilityError: target count, transformations the kernels do not evaluate
    if acqf.supports_multi_output:
        raise IncompatibleAcquisitionFunctionError(
            f"The acquisition function '{type(acqf).__name__}' needs a multi-output objective, but '{kind}' is a single-output "
            f"objective; use qLogExpectedImprovement (the default) or another single-output acquisition function."
        )
    if getattr(acqf, "kind", None) in ("qNEI", "qLogNEI"):
        raise IncompatibilityError(
            f"'{type(acqf).__name__}' under a per-sample desirability scalarisation is not on the HIP path; use "
            f"qLogExpectedImprovement, qExpectedImprovement, qProbabilityOfImprovement, qSimpleRegret, qUpperConfidenceBound or "
            f"qPosteriorStandardDeviation, or BotorchRecommender."
        )
    if getattr(acqf, "is_analytic", False) and program.as_affine() is None:
        # Gaussian only for an arithmetic mean of affine targets (to_botorch_posterior_transform, objectives/desirability.py:266-320)
        raise IncompatibilityError(
            f"The selected analytical acquisition function '{type(acqf).__name__}' is incompatible with the assigned objective "
            f"'{kind}' because the former requires a Gaussian distribution and the latter is configured to produce "
            f"non-Gaussian outcomes."
        )
    return program


def _is_desirability(program) -> bool:
    return type(program).__name__ == "DesirabilityProgram"


def _is_ehvi(acqf) -> bool:
    """qEHVI / qLogEHVI: scored by ``baybe_amd.ehvi.HipEHVI`` (joint q'-batches), not by the baseline-caching noisy scorers."""
    return getattr(acqf, "kind", None) in ("qEHVI", "qLogEHVI")


def _is_nipv(acqf) -> bool:
    """qNIPV: scored by ``baybe_amd.nipv.HipNIPV`` (no samples, no incumbent)."""
    return getattr(acqf, "kind", None) == "qNIPV"


def _nipv_kernel_refusal(surrogate, searchspace):
    """Why the surrogate has no qNIPV kernel on the device (None: it has) - decided from the surrogate's settings and the search
    space's encoding alone, before anything is fitted."""
    from baybe_amd.nipv import NIPV_KERNELS

    use = "use a single Matern-1/2, Matern-3/2, Matern-5/2 or RBF kernel, or BotorchRecommender"
    if not hasattr(surrogate, "kernel_or_factory"):
        return (f"qNIPV on the HIP path needs the Gaussian process surrogate, not '{type(surrogate).__name__}' (forest and linear "
                f"surrogates have no joint posterior to condition); use HipGaussianProcessSurrogate or BotorchRecommender.")
    kernel = surrogate.kernel if surrogate.kernel_or_factory is None else surrogate.kernel_or_factory
    bounds = np.asarray(searchspace.scaling_bounds.to_numpy(), dtype=np.float64)
    d = bounds.shape[1]
    spec = None
    if getattr(surrogate, "preset", "BAYBE") != "BAYBE":
        from baybe_amd.gp_spec import from_preset

        spec = from_preset(surrogate.preset, d, bounds[0], bounds[1])
    elif isinstance(kernel, str):
        name = kernel
    elif callable(kernel) and not hasattr(kernel, "to_gpytorch") and not hasattr(kernel, "lengthscale_prior"):
        return (f"qNIPV on the HIP path must know the kernel before the fit; a kernel factory decides it from the training data; "
                f"{use}.")
    else:
        from baybe_amd.gp_spec import GPSpec
        from baybe_amd.kernels import apply_kernel_spec

        spec = GPSpec.baybe_default(d, bounds[0], bounds[1])
        apply_kernel_spec(spec, kernel, searchspace)
    if spec is not None:
        if spec.n_factors > 1 or spec.has_subsets:
            return (f"qNIPV on the HIP path takes a single kernel over all numerical columns, not a composite kernel or one on a "
                    f"parameter subset; {use}.")
        name = spec.kernel
    if name not in NIPV_KERNELS:
        return (f"qNIPV on the HIP path takes Matern-1/2, Matern-3/2, Matern-5/2 and RBF kernels; the kernel '{name}' (RFF, "
                f"piecewise-polynomial, rational-quadratic, periodic, dot-product) is not among them; {use}.")
    return None


def _polytope_of(cont):
    """The ``Polytope`` of a continuous subspace that carries linear constraints (None: it has none).  Building it checks what the
    device-side sampler and projection take - row and column limits, no interpoint rows, a set with interior - and raises an
    ``IncompatibilityError`` naming the alternative otherwise."""
    if not any(len(getattr(cont, name, ()) or ()) for name in ("constraints_lin_eq", "constraints_lin_ineq")):
        return None
    from baybe_amd.polytope import Polytope

    return Polytope.from_subspace(cont)


def _check_continuous_part(cont, optimizer: str = "compass") -> None:
    """What of ``SubspaceContinuous`` the HIP path's search handles: box-bounded parameters, and under
    ``continuous_optimizer="gradient"`` linear equality / inequality constraints on them (``baybe_amd.polytope``).  Nonlinear /
    cardinality / interpoint constraints need the reference's constrained optimiser.  ``optimizer``: the recommender's
    ``continuous_optimizer``."""
    for name in ("constraints_lin_eq", "constraints_lin_ineq", "constraints_nonlin", "constraints_cardinality"):
        if len(getattr(cont, name, ()) or ()):
            if optimizer == "gradient" and name in ("constraints_lin_eq", "constraints_lin_ineq"):
                continue
            raise IncompatibilityError(
                f"The continuous subspace carries '{name}'; the HIP path searches box-bounded continuous parameters only. "
                f"Use BotorchRecommender."
            )
    dc = len(getattr(getattr(cont, "comp_rep_bounds", None), "columns", ()))
    if optimizer == "gradient":
        if dc > MAX_GRADIENT_CONTINUOUS:  # (before anything is fitted)
            raise IncompatibilityError(
                f"{dc} continuous parameters: continuous_optimizer='gradient' differentiates up to {MAX_GRADIENT_CONTINUOUS} of them "
                f"on the device; use BotorchRecommender beyond that.")
        _polytope_of(cont)  # (before anything is fitted: more than 16 rows, an interpoint row, an empty set)
        return
    if dc > MAX_HYBRID_CONTINUOUS:  # (before anything is fitted)
        raise IncompatibilityError(
            f"{dc} continuous parameters: the HIP path searches the continuous box derivative-free (Sobol raw samples + pattern "
            f"search) and is held to the reference's enumeration (optimize_acqf_mixed) for up to {MAX_HYBRID_CONTINUOUS} of them "
            f"(tests/test_hybrid_gpu.py); use BotorchRecommender, whose gradient optimiser is the tool beyond that.")


def _gradient_kernel_refusal(surrogate, searchspace):
    """Why the surrogate's kernel has no device-side derivative (None: it has) - decided from the surrogate's settings and the
    search space's encoding alone, before anything is fitted."""
    use = "use continuous_optimizer='compass' (up to 4 continuous parameters) or BotorchRecommender"
    if not hasattr(surrogate, "kernel_or_factory"):
        return f"continuous_optimizer='gradient' needs the Gaussian process surrogate, not '{type(surrogate).__name__}'; {use}."
    kernel = surrogate.kernel if surrogate.kernel_or_factory is None else surrogate.kernel_or_factory
    bounds = np.asarray(searchspace.scaling_bounds.to_numpy(), dtype=np.float64)
    d = bounds.shape[1]
    if getattr(surrogate, "preset", "BAYBE") != "BAYBE":
        from baybe_amd.gp_spec import from_preset

        spec = from_preset(surrogate.preset, d, bounds[0], bounds[1])
    elif isinstance(kernel, str):
        spec = None
        name = kernel
    elif callable(kernel) and not hasattr(kernel, "to_gpytorch") and not hasattr(kernel, "lengthscale_prior"):
        return (f"continuous_optimizer='gradient' must know the kernel before the fit; a kernel factory decides it from the training "
                f"data. Pass a Matern-3/2, Matern-5/2 or RBF kernel, or {use}.")
    else:
        from baybe_amd.gp_spec import GPSpec
        from baybe_amd.kernels import apply_kernel_spec

        spec = GPSpec.baybe_default(d, bounds[0], bounds[1])
        apply_kernel_spec(spec, kernel, searchspace)
    if spec is not None:
        if spec.n_factors > 1 or spec.has_subsets:
            return (f"continuous_optimizer='gradient' differentiates a single Matern-3/2, Matern-5/2 or RBF kernel over all numerical "
                    f"columns, not a composite kernel or one on a parameter subset; {use}.")
        name = spec.kernel
    if name not in GRADIENT_KERNELS:
        return (f"continuous_optimizer='gradient' differentiates Matern-3/2, Matern-5/2 and RBF kernels; the kernel '{name}' (RFF, "
                f"piecewise-polynomial, rational-quadratic, periodic, dot-product, Matern-1/2) has no derivative on the device; {use}.")
    return None


def _choose_scorer(model, acqf, program):
    """(path, scorer class) serving a surrogate model, an acquisition function and an objective program - the one place a path is
    chosen: ``_setup_acqf`` builds that scorer, ``_check_batch_size`` asks the class for its cap before anything is fitted.  The
    objective enters through what ``_check_objective`` made of it: ``program``, and a multi-output objective exactly where the
    acquisition function is a multi-output one.  Classes are looked up per call, so that the tests' CPU doubles are found."""
    from baybe_amd import desirability, ehvi, forest, linear, nehvi, nei, nipv, nparego, scoring

    kind, analytic = getattr(acqf, "kind", None), getattr(acqf, "is_analytic", False)
    if getattr(model, "is_independent_gaussian", False):
        return ("linear_analytic", linear.HipLinearAnalytic) if analytic else ("linear", linear.HipLinearAcq)
    if _is_ehvi(acqf):
        return "ehvi", ehvi.HipEHVI
    if _is_nipv(acqf):
        return "nipv", nipv.HipNIPV
    if _is_desirability(program):
        return "desirability", desirability.HipDesirability
    if kind == "qLogNParEGO":
        return "nparego", nparego.HipNParEGO
    if getattr(acqf, "supports_multi_output", False):
        return "nehvi", nehvi.HipNEHVIPlain if kind == "qNEHVI" else nehvi.HipNEHVI
    if kind in ("qNEI", "qLogNEI"):
        return "nei", nei.HipNEI
    if getattr(model, "is_ensemble", False) and not analytic:
        return "forest", forest.HipForestAcq
    return "single", scoring.HipSingleTargetAcq  # (and the analytic kinds on the forest's ensemble moments)


class HipRecommenderImpl:
    """Behaviour of the Bayesian recommender scoring the full discrete candidate set on an MI355X.  No fields: they
    are attached by ``attrs.make_class`` - below for the stand-alone class, in ``baybe_amd.plugin`` on top of BayBE's
    ``BayesianRecommender``, whose ``recommend`` (``pure/bayesian/base.py:130-197``) then drives the overrides
    ``_setup_botorch_acqf`` / ``_recommend_with_discrete_parts`` / ``_recommend_discrete`` defined here."""

    __slots__ = ()

    supports_discrete_subset_generating_constraints: ClassVar[bool] = True
    is_available = _availability_property()

    # ---- copies (simulation/core.py:124, scenarios.py:296, transfer_learning.py:78 deep-copy whole campaigns) --------
    _SHARED_ON_COPY: ClassVar[tuple] = ("_cand_cache", "shard")  # resident candidate matrix (up to 160 MB of HBM): shared, read-only
    _DROPPED_ON_COPY: ClassVar[tuple] = ("_scorer",)  # per-call acquisition state holding device handles: rebuilt by every recommend()

    def __deepcopy__(self, memo):
        from copy import deepcopy

        cls = type(self)
        new = cls.__new__(cls)
        memo[id(self)] = new
        for a in attrs.fields(cls):
            val = getattr(self, a.name)
            if a.name in self._DROPPED_ON_COPY:
                val = None
            elif a.name not in self._SHARED_ON_COPY:
                val = deepcopy(val, memo)
            object.__setattr__(new, a.name, val)
        return new

    def __getstate__(self):
        """Pickling: as ``__deepcopy__``, but the device-resident candidate matrix stays behind too (it is uploaded again
        from the search space on first use)."""
        return {a.name: (None if a.name in self._DROPPED_ON_COPY or a.name == "_cand_cache" else getattr(self, a.name))
                for a in attrs.fields(type(self))}

    def __setstate__(self, state):
        for k, v in state.items():
            object.__setattr__(self, k, v)

    # ---- BayesianRecommender surface -----------------------------------------------------------
    def _get_acquisition_function(self, objective, override=None):
        """Native acquisition spec for the context (default choice: pure/bayesian/base.py:70-74); BayBE's own
        acquisition objects are mapped by class name (``baybe_amd.acquisition.convert_acqf``)."""
        chosen = override if override is not None else self.acquisition_function
        if chosen is None:
            return qLogNoisyExpectedHypervolumeImprovement() if _is_multi_output(objective) else qLogExpectedImprovement()
        return convert_acqf(chosen, ehvi=getattr(self, "ehvi", "refuse"), nipv=getattr(self, "nipv", "refuse"))

    def get_surrogate(self, searchspace, objective, measurements):
        from baybe_amd.surrogates import modeled_quantities

        several = _is_multi_output(objective) or len(modeled_quantities(objective)) > 1  # (desirability: one model per target)
        if several and not self._surrogate_model.supports_multi_output:
            self._surrogate_model = self._surrogate_model.replicate()  # pure/bayesian/base.py:35-39
        self._surrogate_model.fit(searchspace, objective, measurements)
        if self.shard is not None and self.shard.world > 1:
            # every rank fitted the same data, but a fit retry re-samples its start point from the priors (private
            # RNG): rank 0's hyper-parameters are the model on every rank
            model = self._surrogate_model
            for sub in (model.models if isinstance(model, HipCompositeImpl) else [model]):
                params = self.shard.agree(sub.engine.params)
                if self.shard.rank != 0:
                    sub.engine.factorize(params)
        return self._surrogate_model

    def _setup_botorch_acqf(self, searchspace, objective, measurements, pending_experiments=None) -> None:
        """Override point of ``BayesianRecommender.recommend`` (base.py:87-111, called at base.py:166-168): the native
        set-up instead of ``acqf.to_botorch(...)``."""
        self._setup_acqf(searchspace, objective, measurements, pending_experiments)

    def _setup_acqf(self, searchspace, objective, measurements, pending_experiments=None, acquisition_function=None):
        """Native counterpart of ``_setup_botorch_acqf``: the refusals of the surrogate's path (before anything is fitted), the fit
        (cached), the pending rows, and the path's scorer (``baybe_amd.scoring``) with its incumbent."""
        cont = getattr(searchspace, "continuous", None)
        acqf = self._get_acquisition_function(objective, acquisition_function)
        if _is_nipv(acqf):  # (before anything is fitted, whatever the surrogate)
            self._check_nipv_context(searchspace, objective, measurements)
        if self.continuous_optimizer == "gradient" and cont is not None and not getattr(cont, "is_empty", True):
            self._check_gradient_context(searchspace, objective, measurements, acquisition_function)
        self._objective = objective
        if getattr(self._surrogate_model, "is_ensemble", False):
            self._refuse_for_forest(searchspace, objective, acqf)
        elif getattr(self._surrogate_model, "is_independent_gaussian", False):
            self._refuse_for_linear(searchspace, objective, acqf, pending_experiments)
        else:
            self._refuse_for_gp(searchspace, objective, acqf)
        self._acqf_in_use = acqf
        if pending_experiments is not None and not acqf.supports_pending_experiments:
            raise IncompatibleAcquisitionFunctionError(
                f"The chosen acquisition function of type '{type(acqf).__name__}' does not support pending experiments."
            )
        surrogate = self.get_surrogate(searchspace, objective, measurements)
        self._pending_comp = None
        if pending_experiments is not None and len(pending_experiments):
            pend = searchspace.transform(pending_experiments, allow_extra=True)  # _builder.py:326-334
            self._pending_comp = np.ascontiguousarray(pend.to_numpy(dtype=np.float64))
        self._scorer, self._best_f = self._build_scorer(surrogate, searchspace, objective, measurements, acqf)
        return surrogate, acqf

    def _refuse_for_gp(self, searchspace, objective, acqf) -> None:
        """What the Gaussian process paths do not cover, before anything is fitted; sets the objective program."""
        cont = getattr(searchspace, "continuous", None)
        hybrid = cont is not None and not getattr(cont, "is_empty", True)
        if hybrid:
            _check_continuous_part(cont, self.continuous_optimizer)  # hybrid / continuous spaces: box-bounded continuous parameters only
        self._program = _check_objective(objective, acqf, self.desirability)
        if _is_desirability(self._program):
            from baybe_amd.desirability import SHARD_TEXT

            if hybrid:
                raise IncompatibilityError(
                    "Desirability objectives with one model per target are scored over discrete search spaces on the HIP path, not "
                    "hybrid / continuous ones; use 'DesirabilityObjective(as_pre_transformation=True)' or BotorchRecommender.")
            if self.shard is not None:
                raise IncompatibilityError(SHARD_TEXT)
        if _is_ehvi(acqf):
            from baybe_amd.ehvi import MAX_OBJECTIVES, check_alpha, shard_text

            check_alpha(acqf.alpha)
            if len(objective.targets) > MAX_OBJECTIVES:
                raise IncompatibilityError(
                    f"'{type(acqf).__name__}' is scored for 2 to {MAX_OBJECTIVES} targets on the HIP path "
                    f"({len(objective.targets)} given). Use BotorchRecommender.")
            if hybrid:
                raise IncompatibilityError(
                    f"'{type(acqf).__name__}' is scored over discrete search spaces on the HIP path, not hybrid / continuous ones; "
                    f"use BotorchRecommender.")
            if self.shard is not None:
                raise IncompatibilityError(shard_text(type(acqf).__name__))

    def _refuse_beyond_single_output(self, objective, acqf, posterior: str) -> None:
        """The forest and linear surrogates model one target and have no noisy / multi-output acquisition functions."""
        from baybe_amd.exceptions import IncompatibleSurrogateError
        from baybe_amd.surrogates import modeled_quantities

        name = type(self._surrogate_model).__name__
        if _is_multi_output(objective) or len(modeled_quantities(objective)) > 1:
            raise IncompatibleSurrogateError(
                f"'{name}' is a single-output surrogate; multi-target objectives are not on its HIP path. Use BotorchRecommender."
            )
        if acqf.supports_multi_output or getattr(acqf, "kind", None) in ("qNEI", "qLogNEI"):
            raise IncompatibleAcquisitionFunctionError(
                f"The acquisition function '{type(acqf).__name__}' is not on the HIP path of '{name}': its {posterior} "
                f"posterior is scored by qLogEI, qEI, qPI, qSR, qUCB, qPSTD and the analytic acquisition functions."
            )

    def _refuse_for_forest(self, searchspace, objective, acqf) -> None:
        """What the path of an ensemble surrogate (``baybe_amd.forest.HipRandomForestSurrogate``) does not cover, before anything
        is fitted."""
        from baybe_amd.forest import refuse_continuous, shard_text

        refuse_continuous(searchspace)
        name = type(self._surrogate_model).__name__
        if self.shard is not None:
            raise IncompatibilityError(shard_text(name))
        self._refuse_beyond_single_output(objective, acqf, "ensemble")
        self._program = _check_objective(objective, acqf)
        if self._program is not None:
            raise IncompatibilityError(
                f"Target '{objective.targets[0].name}' carries a transformation; the HIP path of '{name}' supports identity "
                f"transformations with optional minimisation only."
            )

    def _refuse_for_linear(self, searchspace, objective, acqf, pending_experiments) -> None:
        """What the path of an independent-Gaussian surrogate (``baybe_amd.linear.HipBayesianLinearSurrogate``) does not cover,
        before anything is fitted.  A transformed single target rides on the objective program, as on the GP path."""
        from baybe_amd.forest import refuse_continuous
        from baybe_amd.linear import refuse_joint, refuse_task_parameters, shard_text

        name = type(self._surrogate_model).__name__
        refuse_task_parameters(searchspace, name)
        refuse_continuous(searchspace)
        self._refuse_beyond_single_output(objective, acqf, "independent Gaussian")
        refuse_joint(name, 1, 0 if pending_experiments is None else len(pending_experiments))
        if self.shard is not None:
            raise IncompatibilityError(shard_text(name))
        self._program = _check_objective(objective, acqf)

    def _build_scorer(self, surrogate, searchspace, objective, measurements, acqf):
        """(scorer, best_f) of the chosen path: its incumbent and its constructor arguments."""
        path, cls = _choose_scorer(self._surrogate_model, acqf, self._program)
        program, beta = self._program, getattr(acqf, "beta", 0.2)

        def measured_rows():  # ALL measurement rows: the noisy forms' baseline (_builder.py:319-324), the incumbent's rows (141-161, 256-265)
            return np.ascontiguousarray(searchspace.transform(measurements, allow_extra=True).to_numpy(dtype=np.float64))

        if path == "desirability":
            engines = [m.engine for m in surrogate.models]
            scorer = cls(engines, program, measured_rows(), acqf.kind, getattr(acqf, "n_mc_samples", 512), beta,
                         device=engines[0].device, analytic=acqf.is_analytic, maximize=getattr(acqf, "maximize", True))
            return scorer, scorer.best_f()  # the desirability of the models' means at all measurement rows
        if path in ("nparego", "nehvi", "ehvi"):
            models = surrogate.models
            engines, signs, X_base = [m.engine for m in models], np.array([m.sign for m in models]), measured_rows()
            if path == "nparego":
                from baybe_amd.nparego import draw_scalarization_weights

                # the weights are fixed when the acquisition function is built: before the scoring and pruning seeds are drawn
                weights = acqf.scalarization_weights
                if weights is None:
                    weights = draw_scalarization_weights(len(models), self.shard.agree if self.shard is not None else None)
                return cls(engines, signs, X_base, weights, n_mc_samples=acqf.n_mc_samples, prune_baseline=acqf.prune_baseline,
                           device=engines[0].device), None
            ref = np.asarray(self._ref_point(acqf, objective, measurements, signs), dtype=np.float64)
            if path == "ehvi":  # the partitioning comes from the models' posterior means at ALL measurement rows (_builder.py:286-299)
                return cls(engines, signs, X_base, ref, log=acqf.kind == "qLogEHVI", n_mc_samples=acqf.n_mc_samples,
                           alpha=acqf.alpha, device=engines[0].device), None
            return cls(engines, signs, X_base, ref, n_mc_samples=acqf.n_mc_samples, prune_baseline=acqf.prune_baseline,
                       device=engines[0].device), None
        eng = surrogate.engine
        sign = 1.0 if program is not None else surrogate.sign  # the kernels' ``sign``: +1 where an objective program carries the orientation
        if path == "nei":  # no incumbent value: the baseline is sampled instead
            return cls(eng, sign, measured_rows(), n_mc_samples=acqf.n_mc_samples, prune_baseline=acqf.prune_baseline,
                       log=acqf.kind == "qLogNEI", device=eng.device), None
        if path == "nipv":
            from baybe_amd.nipv import integration_points

            # the integration points are sampled from ALL rows of the discrete subspace when the acquisition function is built
            P = integration_points(acqf, searchspace, device=eng.device)
            return cls(eng, P.to_numpy(dtype=np.float64), device=eng.device), None
        # _builder.py:141-161, 256-265: the transformed posterior mean at the training inputs
        best_f = eng.best_f(surrogate.sign) if program is None else eng.best_f(1.0, program)
        if path == "forest":
            return cls(surrogate, acqf.kind, sign, best_f, acqf.n_mc_samples, beta), best_f
        if path == "linear":
            return cls(surrogate, acqf.kind, sign, best_f, acqf.n_mc_samples, beta, program), best_f
        return cls(surrogate if path == "linear_analytic" else eng, acqf, sign, best_f, program), best_f

    @staticmethod
    def _ref_point(acqf, objective, measurements, signs):
        ref = acqf.reference_point
        if isinstance(ref, tuple):
            return ref
        from baybe_amd.nehvi import compute_ref_point

        complete = measurements[[t.name for t in objective.targets]].dropna()  # _builder.py:301-317: from completely measured rows
        if complete.empty:
            raise ValueError(
                "For calculating a default reference point, at least one configuration must have a "
                "measured value for all targets. Set 'reference_point' explicitly."
            )
        kw = {} if ref is None else {"factor": ref}
        return compute_ref_point(complete.to_numpy(dtype=np.float64) * signs[None, :], **kw)

    def _check_nipv_context(self, searchspace, objective, measurements) -> None:
        """What qNIPV covers on the device - one untransformed target, a discrete space, a single-task GP with one Matern / RBF
        kernel, at most 512 training points, one device - checked before anything is fitted; every text says what to use instead."""
        from baybe_amd.nipv import MAX_TRAINING_POINTS
        from baybe_amd.surrogates import _target_sign, modeled_quantities

        quantities = modeled_quantities(objective)
        if len(quantities) > 1 and not _is_multi_output(objective) and self.desirability == "device":
            raise IncompatibilityError(
                "qNIPV integrates the posterior variance of ONE model; a DesirabilityObjective with one model per target "
                "(desirability='device') has several. Use 'DesirabilityObjective(as_pre_transformation=True)' or a single target.")
        if len(quantities) == 1 and not _is_multi_output(objective):
            try:
                _target_sign(quantities[0])
            except IncompatibilityError:
                raise IncompatibilityError(
                    "'qNegIntegratedPosteriorVariance' currently does not support any target transformations. Use an untransformed "
                    "target (minimisation is fine: the direction does not enter).") from None
        cont = getattr(searchspace, "continuous", None)
        if cont is not None and not getattr(cont, "is_empty", True):
            raise IncompatibilityError(
                "qNIPV is scored over discrete search spaces on the HIP path (discrete integration points), not hybrid / continuous "
                "ones; use BotorchRecommender.")
        if self.shard is not None:
            raise IncompatibilityError("Row shards are not on the HIP path of qNIPV; score the candidates on one device.")
        if getattr(searchspace, "task_idx", None) is not None or int(getattr(searchspace, "n_tasks", 1)) > 1:
            raise IncompatibilityError("qNIPV on the HIP path handles single-task models, not task parameters; use BotorchRecommender.")
        why = _nipv_kernel_refusal(self._surrogate_model, searchspace)
        if why is not None:
            raise IncompatibilityError(why)
        if measurements is not None and len(measurements) > MAX_TRAINING_POINTS:
            raise IncompatibilityError(
                f"qNIPV on the HIP path conditions models of up to {MAX_TRAINING_POINTS} training points ({len(measurements)} given); "
                f"use BotorchRecommender beyond that.")

    def _check_gradient_context(self, searchspace, objective, measurements, acquisition_function=None) -> None:
        """What ``continuous_optimizer="gradient"`` covers - qLogEI of one untransformed target under a single-task GP with one
        Matern-3/2 / Matern-5/2 / RBF kernel, at most 512 training points, one device - checked before anything is fitted; every
        text says what to use instead."""
        use = "use continuous_optimizer='compass' (up to 4 continuous parameters) or BotorchRecommender"
        _check_continuous_part(searchspace.continuous, "gradient")
        if _is_multi_output(objective):
            raise IncompatibilityError(f"continuous_optimizer='gradient' handles single-target objectives, not multi-output ones; {use}.")
        acqf = self._get_acquisition_function(objective, acquisition_function)
        if getattr(acqf, "kind", None) != "qLogEI":
            raise IncompatibleAcquisitionFunctionError(
                f"continuous_optimizer='gradient' differentiates qLogExpectedImprovement only, not '{type(acqf).__name__}'; {use}.")
        if _check_objective(objective, acqf) is not None:
            raise IncompatibilityError(f"continuous_optimizer='gradient' has no derivative of a transformed target; {use}.")
        if getattr(searchspace, "task_idx", None) is not None or int(getattr(searchspace, "n_tasks", 1)) > 1:
            raise IncompatibilityError(f"continuous_optimizer='gradient' handles single-task models, not task parameters; {use}.")
        why = _gradient_kernel_refusal(self._surrogate_model, searchspace)
        if why is not None:
            raise IncompatibilityError(why)
        if measurements is not None and len(measurements) > MAX_GRADIENT_TRAINING_POINTS:
            raise IncompatibilityError(
                f"continuous_optimizer='gradient' differentiates models of up to {MAX_GRADIENT_TRAINING_POINTS} training points "
                f"({len(measurements)} given); {use}.")
        if self.shard is not None and getattr(self.shard, "world", 1) > 1:
            raise IncompatibilityError(f"continuous_optimizer='gradient' runs on one device, not under row shards; {use}.")

    def _check_batch_size(self, batch_size, pending_experiments=None) -> None:
        """The cap of the chosen path (``check_request``, beside its scorer): the reference has no such limit, so say so before
        any candidate is scored - and, from ``recommend``, before the fit."""
        n_pend = len(self._pending_comp) if self._pending_comp is not None else (
            0 if pending_experiments is None else len(pending_experiments))
        _, cls = _choose_scorer(self._surrogate_model, self._acqf_in_use, self._program)
        cls.check_request(batch_size, n_pend, self._acqf_in_use, self._program, self._surrogate_model)

    def recommend(self, batch_size, searchspace, objective=None, measurements=None, pending_experiments=None) -> pd.DataFrame:
        if objective is None:
            raise NotImplementedError(
                "Recommenders of type 'BayesianRecommender' require that an objective is specified."
            )
        if measurements is None or measurements.empty:
            raise NotImplementedError("Recommenders of type 'BayesianRecommender' do not support empty training data.")
        self._acqf_in_use = self._get_acquisition_function(objective)
        self._pending_comp = None
        if _is_nipv(self._acqf_in_use):  # (its own sentences come first: the reference's for a transformed target among them)
            self._check_nipv_context(searchspace, objective, measurements)
        self._program = _check_objective(objective, self._acqf_in_use, self.desirability)  # (decides the batch-size cap)
        self._check_batch_size(batch_size, pending_experiments)  # before the fit
        self._setup_botorch_acqf(searchspace, objective, measurements, pending_experiments)
        return self._recommend_with_discrete_parts(searchspace, batch_size, pending_experiments=pending_experiments)

    def _recommend_with_discrete_parts(self, searchspace, batch_size, pending_experiments=None) -> pd.DataFrame:
        sd = searchspace.discrete
        self._check_batch_size(batch_size)
        cont = getattr(searchspace, "continuous", None)
        if cont is not None and not getattr(cont, "is_empty", True):  # hybrid space (pure/base.py:268-303)
            if getattr(sd, "is_empty", False):
                return self._recommend_hybrid(searchspace, pd.DataFrame(), batch_size)
            candidates_exp, _ = sd.get_candidates()
            return self._recommend_hybrid(searchspace, candidates_exp, batch_size)
        mask = getattr(sd, "mask_keep", None)  # FilteredSubspaceDiscrete (searchspace/_filtered.py:14-44)
        if (isinstance(mask, np.ndarray) and mask.dtype == bool and len(mask) == len(sd.exp_rep)
                and getattr(sd, "n_subsets", 0) == 0):
            # The candidate set is "the rows of the resident matrix where the keep-mask is set": the mask goes to
            # the device as it is and the two N-row dataframe copies of get_candidates() (50 ms at 1e6 rows) are
            # not made.  Same candidates, same order, same first-index ties.
            if int(mask.sum()) < batch_size:
                raise NotEnoughPointsLeftError(
                    f"Using the current settings, there are fewer than {batch_size} possible data points left to recommend."
                )
            idxs = self._recommend_discrete_without_subsets(sd, None, batch_size, keep_mask=mask)
            return sd.exp_rep.loc[idxs, :]
        candidates_exp, _ = sd.get_candidates()
        if len(candidates_exp) < batch_size:
            raise NotEnoughPointsLeftError(
                f"Using the current settings, there are fewer than {batch_size} possible data points left to recommend."
            )
        idxs = self._recommend_discrete(searchspace.discrete, candidates_exp, batch_size)
        return searchspace.discrete.exp_rep.loc[idxs, :]

    # ---- discrete optimisation -----------------------------------------------------------------
    def _sampler_seed(self, agree: bool = True) -> int:
        """MC sampler seed from torch's global RNG (``engine.draw_sampler_seed``); with row shards rank 0's draw.  The scorers'
        ``seeds`` (``baybe_amd.scoring``); ``agree=False``: this rank's own draw."""
        seed = draw_sampler_seed()
        return int(self.shard.agree(seed)) if agree and self.shard is not None else seed

    def _candidates_on_device(self, subspace_discrete, candidates_exp, keep_mask=None):
        """(X_dev, alive, labels): the *whole* comp rep of the discrete subspace as a device-resident
        fp64 matrix (uploaded once per search space, cached), plus a uint8 mask of the rows that are
        candidates in this call (``None`` = all) and the index labels of the resident rows.

        Campaign.recommend shrinks the candidate set by a few rows per iteration
        (``campaign.py:549-572``); masking instead of re-encoding / re-uploading N x d doubles removes
        the O(N) pandas work and the PCIe copy from every call after the first.
        Row order = search-space order, so first-index tie-breaking is unchanged."""
        import torch

        comp_rep = subspace_discrete.comp_rep
        # The resident copy is keyed on the CONTENT of the comp rep (xxh3 over all N x d doubles: ~10 ms at 1e6 x 20,
        # against 50 ms for re-encoding and re-uploading them), so an edit of any row is noticed
        # (hashed column by column: a column of a numeric frame is a view of its block, whereas ``to_numpy()`` of a frame
        # with one block per column interleaves all N x d values into a new array - 11 ms of every call at 1e6 x 20)
        idx = comp_rep.index
        idx_key = (idx.start, idx.stop, idx.step) if isinstance(idx, pd.RangeIndex) else _content_hash(np.asarray(idx))
        key = (comp_rep.shape, tuple(comp_rep.columns), _frame_content_hash(comp_rep), idx_key)
        if self._cand_cache is None or self._cand_cache[0] != key:
            values = comp_rep.to_numpy(dtype=np.float64)
            X = torch.from_numpy(np.ascontiguousarray(values))
            if self.shard is not None:
                if self.shard.N_total != len(comp_rep):
                    raise ValueError(
                        f"RowShard was built for {self.shard.N_total} rows but the discrete subspace has {len(comp_rep)}"
                    )
                X = X[self.shard.start : self.shard.stop]
            self._cand_cache = (key, X.to(self._engine._dev()), comp_rep.index)
        _, Xd, labels = self._cand_cache
        alive = None
        if keep_mask is not None:
            if not keep_mask.all():
                mask = keep_mask.astype(np.uint8)
                if self.shard is not None:
                    mask = mask[self.shard.start : self.shard.stop]
                alive = torch.from_numpy(mask).to(Xd.device)
        elif len(candidates_exp) != len(labels) or not candidates_exp.index.equals(labels):
            pos = labels.get_indexer(candidates_exp.index)
            if (pos < 0).any():
                raise KeyError("candidates contain rows that are not part of the discrete subspace")
            mask = np.zeros(len(labels), dtype=np.uint8)
            mask[pos] = 1
            if self.shard is not None:
                mask = mask[self.shard.start : self.shard.stop]
            alive = torch.from_numpy(mask).to(Xd.device)
        return Xd, alive, labels

    @property
    def _engine(self):
        model = self._surrogate_model
        return model.models[0].engine if isinstance(model, HipCompositeImpl) else model.engine

    def _recommend_discrete(self, subspace_discrete, candidates_exp: pd.DataFrame, batch_size: int) -> pd.Index:
        assert self._objective is not None
        acqf = self._acqf_in_use
        if batch_size > 1 and not acqf.supports_batching:
            raise IncompatibleAcquisitionFunctionError(
                f"The '{self.__class__.__name__}' only works with Monte Carlo acquisition functions for batch sizes > 1."
            )
        n_sub = getattr(subspace_discrete, "n_subsets", 0)
        if n_sub > 0:
            return self._recommend_discrete_with_subsets(subspace_discrete, candidates_exp, batch_size)
        return self._recommend_discrete_without_subsets(subspace_discrete, candidates_exp, batch_size)

    def _recommend_discrete_without_subsets(self, subspace_discrete, candidates_exp, batch_size, return_values=False,
                                            keep_mask=None):
        Xd, alive, labels = self._candidates_on_device(subspace_discrete, candidates_exp, keep_mask)
        res = self._scorer.select(Xd, batch_size, seeds=self._sampler_seed, X_pending=self._pending_comp, alive=alive,
                                  shard=self.shard)
        idxs = labels[np.asarray(res.indices, dtype=np.int64)]
        return (idxs, res) if return_values else idxs

    def _recommend_discrete_with_subsets(self, subspace_discrete, candidates_exp, batch_size) -> pd.Index:
        """``recommend_discrete_with_subsets`` (botorch/discrete.py:21-75): one greedy run per
        batch-constraint subset, the batch with the highest joint acquisition value wins."""
        if subspace_discrete.n_subsets <= self.max_n_subsets:
            masks = subspace_discrete.subset_masks(candidates_exp, min_candidates=batch_size)
        else:
            masks = subspace_discrete.sample_subset_masks(candidates_exp, self.max_n_subsets, min_candidates=batch_size)
        best = None
        for mask in masks:
            subset = candidates_exp.loc[mask]
            idxs = self._recommend_discrete_without_subsets(subspace_discrete, subset, batch_size)
            comp = subspace_discrete.comp_rep.loc[idxs].to_numpy(dtype=np.float64)
            val = self._joint_value(comp)
            if best is None or val > best[1]:
                best = (idxs, val)
        if best is None:
            from baybe_amd.exceptions import IncompatibilityError as _E

            raise _E("No feasible subset with enough candidates was found.")
        return best[0]

    # ---- hybrid and continuous spaces --------------------------------------------------------------
    def _recommend_hybrid(self, searchspace, candidates_exp: pd.DataFrame, batch_size: int) -> pd.DataFrame:
        """``recommend_hybrid_without_subsets`` (botorch/hybrid.py:30-163) as a data-parallel search.  The reference hands BoTorch's
        ``optimize_acqf_mixed`` one fixed-feature dictionary per discrete row and runs a multi-start gradient optimiser over the
        continuous parameters for each - "a brute-force calculation ... computationally expensive" (its own docstring).  Here the
        brute force is one scoring pass: every discrete candidate row is crossed with ``n_raw_samples`` scrambled-Sobol points of
        the continuous box (the raw samples of BoTorch's initialiser), all rows are scored on the device, and the ``n_restarts`` best
        rows are refined in their continuous coordinates by a compass search (2 d_c probes per start and iteration, all starts in
        one pass, step halved when no probe improves) - no acquisition gradients exist on this path.  Batches are built greedily with
        the chosen points pending, as ``optimize_acqf_mixed`` does.  Same options (``hybrid_sampler`` "Random",
        ``sampling_percentage``, ``n_restarts``, ``n_raw_samples``), same return frame (discrete part in experimental representation,
        indexed by the discrete candidate, plus the continuous columns); purely continuous spaces arrive here through
        ``PureRecommender._recommend_continuous`` with an empty discrete part.  Not a parity path: both sides are stochastic
        multi-start searches, compared by the acquisition value they reach (tests/test_hybrid_*.py)."""
        import torch

        from baybe_amd.engine import GreedyResult  # noqa: F401

        cont, disc = searchspace.continuous, searchspace.discrete
        gradient = self.continuous_optimizer == "gradient"
        _check_continuous_part(cont, self.continuous_optimizer)
        self._last_continuous_trace = []
        acqf, surrogate = self._acqf_in_use, self._surrogate_model
        if not self._scorer.supports_continuous:
            raise IncompatibilityError("Multi-output objectives (qLogNEHVI / qNEHVI / qLogNParEGO) and qNEI / qLogNEI in hybrid / continuous spaces are not on the HIP path; use BotorchRecommender.")
        if batch_size > 1 and not acqf.supports_batching:
            raise IncompatibleAcquisitionFunctionError(
                f"The '{self.__class__.__name__}' only works with Monte Carlo acquisition functions for batch sizes > 1.")
        if getattr(disc, "n_subsets", 0) > 0:
            raise IncompatibilityError("Discrete subset-generating constraints in hybrid spaces are not on the HIP path.")
        eng = surrogate.engine
        cnames = list(cont.comp_rep_bounds.columns)
        cb = cont.comp_rep_bounds.to_numpy(dtype=np.float64)  # [2, d_c]
        dc = len(cnames)
        has_disc = candidates_exp is not None and len(candidates_exp.columns) > 0 and len(candidates_exp) > 0
        if has_disc:
            Dcomp = disc.comp_rep.loc[candidates_exp.index]
            n_keep = int(np.ceil(self.sampling_percentage * len(Dcomp)))
            if self.hybrid_sampler is not None and n_keep < len(Dcomp):
                Dcomp = Dcomp.iloc[self._sample_discrete_rows(Dcomp, n_keep)]
            D = np.ascontiguousarray(Dcomp.to_numpy(dtype=np.float64))
            labels = Dcomp.index
        else:
            D = np.zeros((1, 0))
            labels = pd.RangeIndex(1)
        Nd, dd = D.shape
        # raw samples of the continuous box: scrambled Sobol, as many per discrete row as a few million rows allow.  The reference runs
        # a gradient optimiser per start; this search has only the raw samples and a compass refinement, so the sample count grows
        # with the continuous dimension (512 per dimension) where the row budget allows, and beyond the dimension the
        # search was validated for (tests/test_hybrid_gpu.py: d_c <= 6) it says so
        R = int(max(1, min(max(self.n_raw_samples, 512 * dc), 4_000_000 // max(Nd, 1))))
        dev = eng._dev()
        poly = _polytope_of(cont) if gradient else None
        if poly is not None:
            # linear constraints: the raw samples are uniform in the polytope, one hit-and-run chain each (bbh_polytope_sample; the
            # reference: get_polytope_samples through SubspaceContinuous.sample_uniform, searchspace/continuous.py:544-571)
            Cd = poly.sample(eng, R, seed=self._sampler_seed())
        else:
            sob = torch.quasirandom.SobolEngine(dimension=max(dc, 1), scramble=True, seed=self._sampler_seed())
            U = sob.draw(R, dtype=torch.float64).numpy()[:, :dc]
            Craw = cb[0] + U * (cb[1] - cb[0])
            Cd = torch.from_numpy(np.ascontiguousarray(Craw)).to(dev)
        Dd = torch.from_numpy(D).to(dev)
        X = torch.cat([Dd.repeat_interleave(R, dim=0), Cd.repeat(Nd, 1)], dim=1).contiguous()  # row i R + r = [disc i | cont r]
        base = self._pending_comp if self._pending_comp is not None else np.zeros((0, dd + dc))
        seed = self._sampler_seed()
        mean, var = eng.posterior(X)
        picks, pick_labels = [], []
        for _step in range(batch_size):
            pend = np.vstack([base] + picks) if picks else base
            scores = self._scorer.scores(X, mean, var, pend, seed)
            if gradient:
                best_row = self._gradient_refine(eng, acqf, X, scores, Nd, R, dd, cb, pend, seed, self._scorer.sign, poly)
                picks.append(best_row.reshape(1, -1))
                if has_disc:
                    pick_labels.append(labels[int(np.nonzero((D == best_row[:dd]).all(axis=1))[0][0])])
                continue
            k = int(min(self.n_restarts, X.shape[0], 64))  # (bbh_topk returns at most 64 rows; the reference's n_restarts has no cap)
            _, top = eng.topk(scores, k)
            top = [int(t) for t in top if t >= 0]
            starts = X[torch.as_tensor(top, device=X.device)].cpu().numpy()
            best_row, _ = self._compass_refine(eng, starts, dd, cb, pend, seed, iters=min(96, 24 + 8 * dc))
            picks.append(best_row.reshape(1, -1))
            if has_disc:  # the label of the refined winner's discrete part (copied bit for bit from its start row)
                pick_labels.append(labels[int(np.nonzero((D == best_row[:dd]).all(axis=1))[0][0])])
        out_cont = pd.DataFrame(np.vstack(picks)[:, dd:], columns=[str(c) for c in cnames])
        if has_disc:
            rec_disc = disc.exp_rep.loc[pd.Index(pick_labels)]
            out_cont.index = rec_disc.index
            return pd.concat([rec_disc, out_cont], axis=1)
        return out_cont

    def _sample_discrete_rows(self, Dcomp: pd.DataFrame, n_keep: int) -> list:
        """Positions of the discrete rows a hybrid recommendation enumerates: ``sample_numerical_df(candidates_comp, n, method=
        hybrid_sampler)`` of the reference (botorch/hybrid.py:92-96, utils/sampling_algorithms.py:185-229) - "Random" is pandas' own
        ``DataFrame.sample`` (numpy's global generator, the same draw as the reference's), "FPS" the reference's
        ``farthest_point_sampling`` itself where BayBE is importable (the plug-in lives inside it)."""
        name = str(getattr(self.hybrid_sampler, "value", self.hybrid_sampler))
        if self.shard is not None:  # row shards: every rank must draw the same subsample - the agreed sampler seed, not a global state
            if name != "Random":
                raise IncompatibilityError("hybrid_sampler='FPS' under row shards is not on the HIP path; use 'Random'.")
            return np.random.default_rng(self._sampler_seed()).choice(len(Dcomp), n_keep, replace=False).tolist()
        if name == "Random":
            return Dcomp.reset_index(drop=True).sample(n_keep).index.tolist()
        if name == "FPS":
            try:
                from baybe.utils.sampling_algorithms import farthest_point_sampling  # type: ignore
            except Exception as ex:  # noqa: BLE001
                raise IncompatibilityError("hybrid_sampler='FPS' needs BayBE's own farthest_point_sampling (baybe is not importable here); "
                                           "use 'Random' or sampling_percentage=1.") from ex
            return list(farthest_point_sampling(Dcomp.to_numpy(), n_keep))
        raise ValueError(f"Unrecognized sampling method: '{name}'.")

    def _gradient_refine(self, eng, acqf, X, scores, Nd: int, R: int, dd: int, cb: np.ndarray, pend, seed, sign, poly=None):
        """Gradient-based refinement of one greedy step.  Starts as the reference chooses them, per discrete row its ``n_restarts``
        best raw samples (``optimize_acqf_mixed`` runs ``optimize_acqf`` per fixed-feature dictionary), restricted to the rows with
        the best raw score so that at most ``MAX_GRADIENT_STARTS`` starts advance together; all of them climb qLogEI in their
        continuous coordinates in ``maximize_box``, one device pass (``qlogei_value_grad``) per trial.  With linear constraints
        (``poly``) they climb in ``maximize_polytope``, the device projection (``bbh_polytope_project``) standing where the box
        optimiser clips.  Returns the best final row and leaves starts, final points, values and the number of projection calls on
        ``_last_continuous_trace``."""
        import torch

        from baybe_amd.continuous import maximize_box, maximize_polytope

        if len(pend) > _lib.MAX_PENDING:
            raise IncompatibilityError(
                f"{len(pend)} pending / batch rows exceed the largest joint q-batch continuous_optimizer='gradient' differentiates "
                f"({_lib.MAX_PENDING + 1} points); use continuous_optimizer='compass' or BotorchRecommender.")
        k = int(min(self.n_restarts, R))
        S2 = torch.nan_to_num(scores, nan=-float("inf")).view(Nd, R)
        _, idx = torch.topk(S2, k, dim=1)  # [Nd, k] raw samples of every discrete row
        rows = torch.arange(Nd, device=S2.device)
        max_rows = max(1, MAX_GRADIENT_STARTS // k)
        if Nd > max_rows:
            rows = torch.sort(torch.topk(S2.max(dim=1).values, max_rows).indices).values
        flat = (rows[:, None] * R + idx[rows]).reshape(-1)
        starts_dev = X[flat].contiguous()
        starts = starts_dev.cpu().numpy()
        dc = starts.shape[1] - dd
        cols = np.arange(dd, dd + dc, dtype=np.int32)
        z = sobol_normal_base_samples(acqf.n_mc_samples, 1 + len(pend), seed)
        eng.set_pending(pend if len(pend) else None)
        disc_dev = starts_dev[:, :dd]

        def value_and_grad(C):
            Xc = torch.cat([disc_dev, torch.from_numpy(np.ascontiguousarray(C)).to(disc_dev.device)], dim=1).contiguous()
            val, grad, ok = eng.qlogei_value_grad(Xc, cols, z, self._best_f, sign)
            return val.cpu().numpy(), grad.cpu().numpy(), ok.cpu().numpy()

        project = poly.projector(eng) if poly is not None else None
        try:
            if project is not None:
                res = maximize_polytope(value_and_grad, starts[:, dd:], project)
            else:
                res = maximize_box(value_and_grad, starts[:, dd:], cb[0], cb[1])
        finally:
            eng.set_pending(None)
        final = np.hstack([starts[:, :dd], res.x])
        vals = np.where(np.isfinite(res.values), res.values, -np.inf)
        i = int(np.argmax(vals))
        self._last_continuous_trace.append({"starts": starts, "final": final, "values": res.values.copy(), "best": i,
                                            "iterations": res.iterations, "calls": res.calls,
                                            "projections": project.calls if project is not None else 0})
        return final[i]

    def _compass_refine(self, eng, starts: np.ndarray, dd: int, cb: np.ndarray, pend, seed, iters: int = 24):
        """Compass (pattern) search on the continuous coordinates of ``starts`` [k, d], all starts advancing together: per
        iteration 2 d_c probes per start (plus and minus the start's step along every continuous axis, clipped to the box) are
        scored in ONE device pass; a start moves to its best improving probe, otherwise its step halves.  Returns the best row and
        its value.  (Same base samples for every evaluation: the MC acquisition is a deterministic function of the point.)"""
        k, d = starts.shape
        dc = d - dd
        cur = starts.copy()
        span = cb[1] - cb[0]
        if dc == 0:
            m, v = eng.posterior(cur)
            val = self._scorer.scores(cur, m, v, pend, seed).cpu().numpy()
            i = int(np.argmax(val))
            return cur[i], float(val[i])
        step = np.full(k, 0.125)  # fraction of the box, per start
        m, v = eng.posterior(cur)
        val = self._scorer.scores(cur, m, v, pend, seed).cpu().numpy()
        for _ in range(iters):
            probes = np.repeat(cur, 2 * dc, axis=0)  # [k * 2 dc, d]: start s, axis a, sign
            for a in range(dc):
                for sg, off in ((+1.0, 0), (-1.0, 1)):
                    rows = np.arange(k) * 2 * dc + 2 * a + off
                    probes[rows, dd + a] = np.clip(cur[:, dd + a] + sg * step * span[a], cb[0, a], cb[1, a])
            pm, pv = eng.posterior(probes)
            pval = self._scorer.scores(probes, pm, pv, pend, seed).cpu().numpy().reshape(k, 2 * dc)
            j = pval.argmax(axis=1)
            better = pval[np.arange(k), j] > val
            rows = np.arange(k) * 2 * dc + j
            cur[better] = probes[rows[better]]
            val[better] = pval[np.arange(k), j][better]
            step[~better] *= 0.5
            if (step < 1e-5).all():  # every start has converged to 1e-5 of the box
                break
        i = int(np.argmax(val))
        return cur[i], float(val[i])

    # ---- read-backs (Campaign.acquisition_values / joint_acquisition_value) ---------------------
    def _joint_value(self, comp: np.ndarray) -> float:
        """The acquisition value of one q-batch, given the pending rows."""
        return self._scorer.joint_value(comp, seeds=self._sampler_seed, X_pending=self._pending_comp)

    def acquisition_values(self, candidates: pd.DataFrame, searchspace, objective, measurements,
                           pending_experiments=None, acquisition_function=None) -> pd.Series:
        """``BayesianRecommender.acquisition_values`` (base.py:199-238): one value per candidate."""
        self._setup_acqf(searchspace, objective, measurements, pending_experiments, acquisition_function)
        comp = np.ascontiguousarray(searchspace.transform(candidates, allow_extra=True).to_numpy(dtype=np.float64))
        scores = self._scorer.values(comp, seeds=self._sampler_seed, X_pending=self._pending_comp)
        return pd.Series(scores.cpu().numpy(), index=candidates.index)

    def joint_acquisition_value(self, candidates: pd.DataFrame, searchspace, objective, measurements,
                                pending_experiments=None, acquisition_function=None) -> float:
        """``BayesianRecommender.joint_acquisition_value`` (base.py:240-269)."""
        self._setup_acqf(searchspace, objective, measurements, pending_experiments, acquisition_function)
        comp = np.ascontiguousarray(searchspace.transform(candidates, allow_extra=True).to_numpy(dtype=np.float64))
        return self._joint_value(comp)


def _convert_hybrid_sampler(value):
    """``DiscreteSamplingMethod`` (utils/sampling_algorithms.py:175-182) by value or member; None = no sampling."""
    if value is None:
        return None
    name = str(getattr(value, "value", value))
    if name not in ("Random", "FPS"):
        raise ValueError(f"'{value}' is not a valid DiscreteSamplingMethod (Random, FPS)")
    return value


def _convert_continuous_optimizer(value):
    """How the continuous coordinates of a hybrid / continuous recommendation are refined: "compass" (derivative-free pattern
    search, up to 4 continuous parameters) or "gradient" (device-side derivatives, up to 32)."""
    name = str(getattr(value, "value", value))
    if name not in ("compass", "gradient"):
        raise ValueError(f"'{value}' is not a valid continuous_optimizer (compass, gradient)")
    return name


def _convert_desirability(value):
    """What happens to a ``DesirabilityObjective`` with one model per target (its default): "refuse" names the alternatives,
    "device" scores the per-sample scalarisation on the device (``baybe_amd.desirability``)."""
    name = str(getattr(value, "value", value))
    if name not in ("refuse", "device"):
        raise ValueError(f"'{value}' is not a valid desirability setting (refuse, device)")
    return name


def _convert_ehvi(value):
    """What happens to qEHVI / qLogEHVI: "refuse" names the alternatives (and the setting), "device" scores them on the device
    (``baybe_amd.ehvi``)."""
    name = str(getattr(value, "value", value))
    if name not in ("refuse", "device"):
        raise ValueError(f"'{value}' is not a valid ehvi setting (refuse, device)")
    return name


def _convert_nipv(value):
    """What happens to qNIPV: "refuse" names the setting, "device" scores it on the device (``baybe_amd.nipv``)."""
    name = str(getattr(value, "value", value))
    if name not in ("refuse", "device"):
        raise ValueError(f"'{value}' is not a valid nipv setting (refuse, device)")
    return name


def _convert_acqf_field(value, self):
    return convert_acqf(value, ehvi=getattr(self, "ehvi", "refuse"), nipv=getattr(self, "nipv", "refuse"))


def _validate_percentage(_, attribute, value):
    if not 0 <= value <= 1:  # botorch/core.py:123-135
        raise ValueError(f"Hybrid sampling percentage needs to be between 0 and 1 but is {value}")


def recommender_fields(with_base_fields: bool = True, surrogate_factory=HipGaussianProcessSurrogate) -> dict:
    """attrs fields of the recommender.  ``with_base_fields=False`` leaves out what BayBE's ``BayesianRecommender``
    declares itself (``acquisition_function``, ``_objective``; pure/bayesian/base.py:46-66); ``_surrogate_model`` is
    redeclared in both cases because its default is the HIP surrogate."""
    f = {
        "_surrogate_model": field(alias="surrogate_model", factory=surrogate_factory),
        "max_n_subsets": field(default=10, validator=[instance_of(int), ge(1)], kw_only=True),  # botorch/core.py:93-98
        # The reference's options for continuous / hybrid optimisation (botorch/core.py:69-91), accepted with its defaults and
        # validators so that constructor calls carry over; none of them affects purely discrete optimisation (the reference says so
        # for n_restarts / n_raw_samples), which is the only kind of search space this recommender takes.
        "sequential_continuous": field(default=True, validator=instance_of(bool), kw_only=True),
        "hybrid_sampler": field(default=None, converter=_convert_hybrid_sampler, kw_only=True),
        "sampling_percentage": field(default=1.0, validator=_validate_percentage, kw_only=True),
        "n_restarts": field(default=10, validator=[instance_of(int), gt(0)], kw_only=True),
        "n_raw_samples": field(default=64, validator=[instance_of(int), gt(0)], kw_only=True),
        # refinement of the continuous coordinates: the pattern search, or - opt-in - gradient ascent on device-side derivatives
        "continuous_optimizer": field(default="compass", converter=_convert_continuous_optimizer, kw_only=True),
        # DesirabilityObjective with one model per target: refused (naming the alternatives), or - opt-in - scored per sample on the device
        "desirability": field(default="refuse", converter=_convert_desirability, kw_only=True),
        # qEHVI / qLogEHVI: refused (naming the setting), or - opt-in - scored on the device by joint q'-batch inclusion-exclusion
        "ehvi": field(default="refuse", converter=_convert_ehvi, kw_only=True),
        # qNIPV (active learning): refused (naming the setting), or - opt-in - scored on the device over discrete search spaces
        "nipv": field(default="refuse", converter=_convert_nipv, kw_only=True),
        # optional baybe_amd.distributed.RowShard: this process scores only its row range and joins one all-gather
        # per selection step (multi-GPU)
        "shard": field(default=None, eq=False, repr=False, kw_only=True),
        "_best_f": field(default=None, init=False, eq=False, repr=False),
        "_pending_comp": field(default=None, init=False, eq=False, repr=False),
        "_cand_cache": field(default=None, init=False, eq=False, repr=False),
        "_scorer": field(default=None, init=False, eq=False, repr=False),
        "_acqf_in_use": field(default=None, init=False, eq=False, repr=False),
        "_program": field(default=None, init=False, eq=False, repr=False),  # ObjectiveProgram of a transformed single target, or a DesirabilityProgram
        # per greedy step of the last hybrid / continuous recommendation under "gradient": starts, final points, values, projection calls (tests, timing)
        "_last_continuous_trace": field(default=None, init=False, eq=False, repr=False),
    }
    if with_base_fields:
        # (converted under the instance's ``ehvi`` / ``nipv`` settings, which are declared - and therefore set - before it)
        f["acquisition_function"] = field(default=None, converter=attrs.Converter(_convert_acqf_field, takes_self=True), kw_only=True)
        f["_objective"] = field(default=None, init=False, eq=False, repr=False)
    return f


HipBotorchRecommender = attrs.make_class("HipBotorchRecommender", recommender_fields(), bases=(HipRecommenderImpl,),
                                         kw_only=True, slots=False)
HipBotorchRecommender.__doc__ = "Bayesian recommender scoring the full discrete candidate set on an MI355X (stand-alone)."
HipBotorchRecommender.__module__ = __name__
HipBotorchRecommender.compatibility = "HYBRID"
