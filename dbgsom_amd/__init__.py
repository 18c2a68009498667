"""MI355X-native batch-SOM training core with the DBGSOM estimator surface.

    from dbgsom_amd import SomVQ, SomClassifier, SomRegressor
"""
from .backend import EpochResult, HipBackend, HotPathBackend  # noqa: F401
from .som_classifier import SomClassifier  # noqa: F401
from .som_regressor import SomRegressor  # noqa: F401
from .som_vq import SomVQ  # noqa: F401

__all__ = ["SomVQ", "SomClassifier", "SomRegressor", "HipBackend", "HotPathBackend", "EpochResult"]
