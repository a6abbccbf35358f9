"""The reconstruction classes.  DenseReconstructor and the method it is built on are resolved lazily, so importing
the package for the camera types does not import the engine."""
__all__ = ["DenseReconstructor", "SfMPipeline", "reconstruct_from_features", "FeatureMatcher", "ImageFeatures", "FeatureMatch",
           "FeatureExtractor", "SiftFeatures",
           "register_view", "refine_pose", "compute_essential_matrix", "decompose_essential", "relative_pose",
           "triangulate_points", "compute_reprojection_error", "find_best_initial_pair", "bundle_adjust", "reprojection_errors"]


def __getattr__(name):
    if name == "DenseReconstructor":
        from .dense import DenseReconstructor
        return DenseReconstructor
    if name == "SfMPipeline":
        from .sfm_pipeline import SfMPipeline
        return SfMPipeline
    if name == "reconstruct_from_features":
        from .dense import DenseReconstructor
        return DenseReconstructor.reconstruct_from_features
    if name in ("FeatureMatcher", "ImageFeatures", "FeatureMatch", "FeatureExtractor", "SiftFeatures"):
        from . import features
        return getattr(features, name)
    if name in ("register_view", "refine_pose"):
        from . import registration
        return getattr(registration, name)
    if name in ("compute_essential_matrix", "decompose_essential", "relative_pose", "triangulate_points",
                "compute_reprojection_error", "find_best_initial_pair"):
        from . import geometry
        return getattr(geometry, name)
    if name in ("bundle_adjust", "reprojection_errors"):
        from . import bundle
        return getattr(bundle, name)
    raise AttributeError(name)
