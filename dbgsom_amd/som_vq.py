"""Unsupervised estimator: vector quantisation / clustering with a growing SOM.

Mirrors ``dbgsom/SomVQ.py`` of the reference (:16-152): ``fit`` / ``predict`` / ``fit_predict``
(from ``ClusterMixin``) / ``labels_``; a sample's label is the index of its best matching unit.
``predict`` and ``fit_predict`` of a device array (see ``base``) return an int64 tensor on its device.
"""
from __future__ import annotations

import numpy as np
from sklearn.base import ClusterMixin, TransformerMixin
from sklearn.utils.validation import check_is_fitted

from .backend import is_device_array
from .base import BaseSom


class SomVQ(BaseSom, ClusterMixin, TransformerMixin):
    """Directed batch growing SOM used as a vector quantiser (see ``BaseSom`` for parameters)."""

    def _check_input_data(self, X, y=None):
        # float32 is kept as float32 (the device stores it as such); anything else -> float64
        # (the finite check rides on the device's column sums when it can: BaseSom._assert_finite_from_moments)
        # (missing_values="nan-fit": NaN passes in dense X -- BaseSom._check_fit_array)
        X, _ = self._check_fit_array(X)
        X = self._check_sparse_input(X)
        return X, None  # any y is ignored

    def _label_prototypes(self, X, y=None) -> None:
        self._lattice.write_attributes({"label": np.arange(len(self._lattice))})

    def predict(self, X) -> np.ndarray:
        """Index of the closest prototype for every sample (SomVQ.py:130-148)."""
        check_is_fitted(self)
        if self._is_resident(X):
            return self._resident_winners(X)
        # integer / half input is converted like the reference's engine does (sklearn's
        # NearestNeighbors); float32 stays float32.  A device array gives a tensor on its device.
        X = self._check_query(X)
        _, labels = self._get_winning_neurons(X, n_bmu=1)
        return labels

    def _fit(self, X) -> None:
        self.labels_ = self.predict(X)

    def fit_predict(self, X, y=None, sample_weight=None) -> np.ndarray:
        """``fit(X, y, sample_weight).labels_``: the index of the best matching unit of every row of X."""
        labels = self.fit(X, y, sample_weight=sample_weight).labels_
        return self._like(labels, X) if is_device_array(X) else labels
