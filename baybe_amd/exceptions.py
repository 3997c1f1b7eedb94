"""Exception types at the plug-in boundary.  When BayBE is importable its own classes are
re-exported (``baybe/exceptions.py:50-178``) so that ``Campaign.recommend`` catches exactly what
it expects (``campaign.py:602-630``); otherwise same-named stand-ins are defined."""

try:  # pragma: no cover - baybe is not importable in the build container
    from baybe.exceptions import (  # type: ignore
        IncompatibilityError,
        IncompatibleAcquisitionFunctionError,
        IncompatibleArgumentError,
        IncompatibleSurrogateError,
        ModelNotTrainedError,
        NotEnoughPointsLeftError,
        UnusedObjectWarning,
    )
except Exception:  # noqa: BLE001

    class IncompatibilityError(Exception):
        """Incompatible components are used together."""

    class IncompatibleSurrogateError(IncompatibilityError):
        """An incompatible surrogate was selected."""

    class IncompatibleAcquisitionFunctionError(IncompatibilityError):
        """An incompatible acquisition function was selected."""

    class IncompatibleArgumentError(IncompatibilityError):
        """An incompatible argument was passed to a callable."""

    class UnusedObjectWarning(UserWarning):
        """A method or function was called with undesired arguments which indicates an unintended user fault."""

    class NotEnoughPointsLeftError(Exception):
        """More recommendations are requested than there are viable candidates left."""

    class ModelNotTrainedError(Exception):
        """A model was used before being trained."""


try:  # pragma: no cover - (older BayBE versions have no insights package)
    from baybe.exceptions import IncompatibleExplainerError, NoMeasurementsError  # type: ignore
except Exception:  # noqa: BLE001

    class IncompatibleExplainerError(IncompatibilityError):
        """An explainer is incompatible with the data it is presented."""

    class NoMeasurementsError(Exception):
        """A context expected measurements but none were available."""


from baybe_amd.engine import ModelFittingError  # noqa: E402,F401
