"""The reconstruction classes.  DenseReconstructor and the method it is built on are resolved lazily, so importing
the package for the camera types does not import the engine."""
__all__ = ["DenseReconstructor", "reconstruct_from_features", "FeatureMatcher", "ImageFeatures", "FeatureMatch",
           "register_view", "refine_pose"]


def __getattr__(name):
    if name == "DenseReconstructor":
        from .dense import DenseReconstructor
        return DenseReconstructor
    if name == "reconstruct_from_features":
        from .dense import DenseReconstructor
        return DenseReconstructor.reconstruct_from_features
    if name in ("FeatureMatcher", "ImageFeatures", "FeatureMatch"):
        from . import features
        return getattr(features, name)
    if name in ("register_view", "refine_pose"):
        from . import registration
        return getattr(registration, name)
    raise AttributeError(name)
