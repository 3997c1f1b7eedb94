"""BayBE's own types for the HIP path: genuine subclasses of ``baybe.surrogates.base.Surrogate`` and
``baybe.recommenders.pure.bayesian.base.BayesianRecommender``.

Why subclasses: ``Campaign.get_surrogate`` / ``acquisition_values`` demand
``isinstance(recommender, BayesianRecommender)`` (``campaign.py:750-807``), the serialisation registry finds
subclasses only (``serialization/core.py:109-146``), and BayBE's test loops enumerate subclasses and construct them as
``cls()`` (``tests/test_iterations.py:75-105``).

How: ``Surrogate`` is a *slotted* attrs class (``surrogates/base.py:81-82``); a second slotted attrs base cannot be
mixed in ("multiple bases have instance lay-out conflict").  The behaviour therefore lives in field-less mixins
with empty ``__slots__`` (``baybe_amd.surrogates.HipGPSurrogateImpl``, ``baybe_amd.recommenders.HipRecommenderImpl``)
and ``attrs.make_class`` attaches the fields on top of BayBE's base, which keeps contributing its own runtime
fields (``_searchspace``, ``_objective``, ``_measurements_hash``; ``acquisition_function``, ``_objective``).  The
mixin comes first in the MRO, so its ``fit`` / ``_setup_botorch_acqf`` / ``_recommend_discrete`` ... override the
base's, while ``BayesianRecommender.recommend`` itself (validation, dataframe preprocessing, ``Settings`` context,
``pure/bayesian/base.py:130-197``) is BayBE's own code driving those overrides.

``tests/test_plugin_layout_cpu.py`` builds the classes on replicas of the two bases that copy their attrs / slots
layout and call flow (BayBE itself cannot be imported in the build container: no ``cattrs``).
"""

from __future__ import annotations

import attrs

from baybe_amd.recommenders import HipRecommenderImpl, recommender_fields
from baybe_amd.sampling import HipFPSRecommenderImpl, fps_recommender_fields
from baybe_amd.surrogates import HipCompositeImpl, HipGPSurrogateImpl, composite_fields, gp_surrogate_fields


def make_baybe_classes(surrogate_base=None, recommender_base=None, discrete_compatibility=None):
    """(HipGaussianProcessSurrogate, HipCompositeSurrogate, HipBotorchRecommender) as subclasses of BayBE's bases.

    Without arguments the bases are imported from ``baybe``; the parameters exist so that the layout can be tested
    against replicas of those bases where ``baybe`` is not importable."""
    if surrogate_base is None:
        from baybe.surrogates.base import Surrogate as surrogate_base
    if recommender_base is None:
        from baybe.recommenders.pure.bayesian.base import BayesianRecommender as recommender_base
    if discrete_compatibility is None:
        from baybe.searchspace.core import SearchSpaceType

        discrete_compatibility = SearchSpaceType.HYBRID  # discrete, hybrid and (through the hybrid fallback) continuous spaces

    surrogate = attrs.make_class("HipGaussianProcessSurrogate", gp_surrogate_fields(with_runtime_state=False),
                                 bases=(HipGPSurrogateImpl, surrogate_base), slots=True)
    surrogate.__doc__ = "A Gaussian process surrogate evaluated on an MI355X (``baybe.surrogates.base.Surrogate``)."
    # the per-target replication of the HIP path keeps the engines resident; it is not BayBE's CompositeSurrogate
    # (deep copies of a template wrapped into a BoTorch ModelListGP, surrogates/composite.py:101-134)
    composite = attrs.make_class("HipCompositeSurrogate", composite_fields(surrogate), bases=(HipCompositeImpl,), slots=True)
    surrogate._composite_class = composite

    recommender = attrs.make_class(
        "HipBotorchRecommender", recommender_fields(with_base_fields=False, surrogate_factory=surrogate),
        bases=(HipRecommenderImpl, recommender_base), kw_only=True, slots=False)
    recommender.__doc__ = ("Bayesian recommender scoring the full discrete candidate set on an MI355X "
                           "(``baybe.recommenders.pure.bayesian.base.BayesianRecommender``).")
    recommender.compatibility = discrete_compatibility
    # BayBE's recommend() (argument validation, dataframe preprocessing, Settings context) stays in charge; it calls
    # _setup_botorch_acqf and, through PureRecommender.recommend, _recommend_with_discrete_parts - both overridden
    recommender.recommend = recommender_base.recommend
    for cls in (surrogate, composite, recommender):
        cls.__module__ = __name__
    return surrogate, composite, recommender


def make_baybe_forest_surrogate(surrogate_base=None):
    """``HipRandomForestSurrogate`` as a subclass of BayBE's ``Surrogate``: the counterpart of ``RandomForestSurrogate``
    (``baybe/surrogates/random_forest.py:59-144``), built exactly as ``make_baybe_classes`` builds the GP surrogate - the field-less
    mixin first in the MRO, the base contributing its runtime fields (``_searchspace``, ``_objective``, ``_measurements_hash``).  Use
    it as ``HipBotorchRecommender(surrogate_model=HipRandomForestSurrogate())``.

    Without an argument the base is imported from ``baybe``; the parameter exists so that the layout can be tested against a replica."""
    from baybe_amd.forest import HipForestSurrogateImpl, forest_surrogate_fields

    if surrogate_base is None:
        from baybe.surrogates.base import Surrogate as surrogate_base
    surrogate = attrs.make_class("HipRandomForestSurrogate", forest_surrogate_fields(with_runtime_state=False),
                                 bases=(HipForestSurrogateImpl, surrogate_base), slots=True)
    surrogate.__doc__ = "A random forest surrogate scored on an MI355X (``baybe.surrogates.base.Surrogate``)."
    surrogate.__module__ = __name__
    return surrogate


def make_baybe_linear_surrogate(surrogate_base=None):
    """``HipBayesianLinearSurrogate`` as a subclass of BayBE's ``Surrogate``: the counterpart of ``BayesianLinearSurrogate``
    (``baybe/surrogates/linear.py:39-94``), built as ``make_baybe_forest_surrogate`` builds the forest - the field-less mixin first in
    the MRO, the base contributing its runtime fields.  Use it as ``HipBotorchRecommender(surrogate_model=HipBayesianLinearSurrogate())``.

    Without an argument the base is imported from ``baybe``; the parameter exists so that the layout can be tested against a replica."""
    from baybe_amd.linear import HipLinearSurrogateImpl, linear_surrogate_fields

    if surrogate_base is None:
        from baybe.surrogates.base import Surrogate as surrogate_base
    surrogate = attrs.make_class("HipBayesianLinearSurrogate", linear_surrogate_fields(with_runtime_state=False),
                                 bases=(HipLinearSurrogateImpl, surrogate_base), slots=True)
    surrogate.__doc__ = "A Bayesian linear (ARD) surrogate scored on an MI355X (``baybe.surrogates.base.Surrogate``)."
    surrogate.__module__ = __name__
    return surrogate


def make_baybe_fps_recommender(base=None, discrete_compatibility=None):
    """``HipFPSRecommender`` as a subclass of BayBE's ``NonPredictiveRecommender``
    (``baybe/recommenders/pure/nonpredictive/base.py:17-58``): the counterpart of BayBE's ``FPSRecommender`` for the first,
    model-free batch of a campaign, e.g. ``TwoPhaseMetaRecommender(initial_recommender=HipFPSRecommender(),
    recommender=HipBotorchRecommender())``.  The base's ``recommend`` (refusal of pending experiments, warnings about unused
    measurements / objective, candidate extraction) stays in charge and calls the overridden ``_recommend_discrete``.

    Without arguments the base is imported from ``baybe``; the parameters exist so that the layout can be tested against a replica."""
    if base is None:
        from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender as base
    if discrete_compatibility is None:
        from baybe.searchspace.core import SearchSpaceType

        discrete_compatibility = SearchSpaceType.DISCRETE
    recommender = attrs.make_class("HipFPSRecommender", fps_recommender_fields(), bases=(HipFPSRecommenderImpl, base), slots=False)
    recommender.__doc__ = ("Initial recommender selecting candidates by farthest point sampling on an MI355X "
                           "(``baybe.recommenders.pure.nonpredictive.base.NonPredictiveRecommender``).")
    recommender.compatibility = discrete_compatibility
    recommender.__module__ = __name__
    return recommender


def make_baybe_pam_recommender(base=None, discrete_compatibility=None):
    """``HipPAMClusteringRecommender`` as a subclass of BayBE's ``NonPredictiveRecommender``: the counterpart of BayBE's
    ``PAMClusteringRecommender`` (``baybe/recommenders/pure/nonpredictive/clustering.py:148-193``), built exactly as
    ``make_baybe_fps_recommender`` builds its class - the base's ``recommend`` stays in charge and calls the overridden
    ``_recommend_discrete``.

    Without arguments the base is imported from ``baybe``; the parameters exist so that the layout can be tested against a replica."""
    from baybe_amd.clustering import HipPAMRecommenderImpl, pam_recommender_fields

    if base is None:
        from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender as base
    if discrete_compatibility is None:
        from baybe.searchspace.core import SearchSpaceType

        discrete_compatibility = SearchSpaceType.DISCRETE
    recommender = attrs.make_class("HipPAMClusteringRecommender", pam_recommender_fields(), bases=(HipPAMRecommenderImpl, base), slots=False)
    recommender.__doc__ = ("Initial recommender selecting the medoids of a k-medoids clustering on an MI355X "
                           "(``baybe.recommenders.pure.nonpredictive.base.NonPredictiveRecommender``).")
    recommender.compatibility = discrete_compatibility
    recommender.__module__ = __name__
    return recommender


def make_baybe_kmeans_recommender(base=None, discrete_compatibility=None):
    """``HipKMeansClusteringRecommender`` as a subclass of BayBE's ``NonPredictiveRecommender``: the counterpart of BayBE's
    ``KMeansClusteringRecommender`` (``baybe/recommenders/pure/nonpredictive/clustering.py:196-252``), built exactly as
    ``make_baybe_pam_recommender`` builds its class - the base's ``recommend`` stays in charge and calls the overridden
    ``_recommend_discrete``.

    Without arguments the base is imported from ``baybe``; the parameters exist so that the layout can be tested against a replica."""
    from baybe_amd.clustering import HipKMeansRecommenderImpl, kmeans_recommender_fields

    if base is None:
        from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender as base
    if discrete_compatibility is None:
        from baybe.searchspace.core import SearchSpaceType

        discrete_compatibility = SearchSpaceType.DISCRETE
    recommender = attrs.make_class("HipKMeansClusteringRecommender", kmeans_recommender_fields(), bases=(HipKMeansRecommenderImpl, base),
                                   slots=False)
    recommender.__doc__ = ("Initial recommender selecting the member nearest to each centre of a k-means clustering on an MI355X "
                           "(``baybe.recommenders.pure.nonpredictive.base.NonPredictiveRecommender``).")
    recommender.compatibility = discrete_compatibility
    recommender.__module__ = __name__
    return recommender


def make_baybe_gmm_recommender(base=None, discrete_compatibility=None):
    """``HipGaussianMixtureClusteringRecommender`` as a subclass of BayBE's ``NonPredictiveRecommender``: the counterpart of BayBE's
    ``GaussianMixtureClusteringRecommender`` (``baybe/recommenders/pure/nonpredictive/clustering.py:255-304``), built exactly as
    ``make_baybe_pam_recommender`` builds its class - the base's ``recommend`` stays in charge and calls the overridden
    ``_recommend_discrete``.

    Without arguments the base is imported from ``baybe``; the parameters exist so that the layout can be tested against a replica."""
    from baybe_amd.clustering import HipGMMRecommenderImpl, gmm_recommender_fields

    if base is None:
        from baybe.recommenders.pure.nonpredictive.base import NonPredictiveRecommender as base
    if discrete_compatibility is None:
        from baybe.searchspace.core import SearchSpaceType

        discrete_compatibility = SearchSpaceType.DISCRETE
    recommender = attrs.make_class("HipGaussianMixtureClusteringRecommender", gmm_recommender_fields(), bases=(HipGMMRecommenderImpl, base),
                                   slots=False)
    recommender.__doc__ = ("Initial recommender selecting a random member of every component of a Gaussian mixture clustering on an "
                           "MI355X (``baybe.recommenders.pure.nonpredictive.base.NonPredictiveRecommender``).")
    recommender.compatibility = discrete_compatibility
    recommender.__module__ = __name__
    return recommender
