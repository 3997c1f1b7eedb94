"""baybe_amd — MI355X-native GP recommend() hot path for BayBE (HIP kernels behind a C-ABI).

Only what the path needs lives here: ``csrc/`` (HIP kernels + the C-ABI of
``include/baybe_hip.h``), the ctypes binding, the host driver (``engine``), and the host-side
mirror of BayBE's surrogate / recommender plug-in surface (``surrogates``, ``recommenders``).
"""

from baybe_amd._lib import HipError, HipUnavailableError, is_available, library_path



def __getattr__(name):
    """``farthest_point_sampling`` / ``HipFPSRecommender`` (``baybe_amd.sampling``) and ``k_medoids`` / ``HipPAMClusteringRecommender`` /
    ``k_means`` / ``HipKMeansClusteringRecommender`` / ``gaussian_mixture`` / ``HipGaussianMixtureClusteringRecommender``
    (``baybe_amd.clustering``) and ``HipRandomForestSurrogate`` / ``make_baybe_forest_surrogate`` (``baybe_amd.forest``,
    ``baybe_amd.plugin``) and ``HipBayesianLinearSurrogate`` / ``make_baybe_linear_surrogate`` (``baybe_amd.linear``,
    ``baybe_amd.plugin``) and ``HipSHAPInsight`` / ``shapley_values`` (``baybe_amd.insights``), imported on first use: the modules pull in pandas and attrs, which a plain ``import baybe_amd`` does
    not need."""
    if name in ("farthest_point_sampling", "HipFPSRecommender"):
        from baybe_amd import sampling

        return getattr(sampling, name)
    if name in ("k_medoids", "HipPAMClusteringRecommender", "k_means", "HipKMeansClusteringRecommender", "gaussian_mixture",
                "HipGaussianMixtureClusteringRecommender"):
        from baybe_amd import clustering

        return getattr(clustering, name)
    if name in ("HipRandomForestSurrogate", "make_baybe_forest_surrogate"):  # (scikit-learn is imported by the first fit only)
        if name == "HipRandomForestSurrogate":
            from baybe_amd import forest

            return forest.HipRandomForestSurrogate
        from baybe_amd import plugin

        return plugin.make_baybe_forest_surrogate
    if name == "HipBayesianLinearSurrogate":  # (scikit-learn is imported by the first fit only)
        from baybe_amd import linear

        return linear.HipBayesianLinearSurrogate
    if name == "make_baybe_linear_surrogate":
        from baybe_amd import plugin

        return plugin.make_baybe_linear_surrogate
    if name in ("HipSHAPInsight", "shapley_values"):
        from baybe_amd import insights

        return getattr(insights, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["HipError", "HipUnavailableError", "is_available", "library_path", "farthest_point_sampling", "HipFPSRecommender", "k_medoids",
           "HipPAMClusteringRecommender", "k_means", "HipKMeansClusteringRecommender", "gaussian_mixture",
           "HipGaussianMixtureClusteringRecommender", "HipRandomForestSurrogate", "make_baybe_forest_surrogate",
           "HipBayesianLinearSurrogate", "make_baybe_linear_surrogate", "HipSHAPInsight", "shapley_values"]
__version__ = "0.1.0"
