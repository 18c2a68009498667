"""Supervised estimator: growing SOM with per-prototype class statistics.

Mirrors ``dbgsom/SomClassifier.py`` of the reference (:19-220).  The training path is the same
accelerated hot path; prototype labelling uses one more BMU pass; ``predict`` /
``predict_proba`` go through the LARS sparse code of ``transform`` exactly as the reference does,
computed by the backend (on the MI355X: csrc/sparse_code.hip).
"""
from __future__ import annotations

from statistics import mode

import numpy as np
from sklearn.base import ClassifierMixin, TransformerMixin
from sklearn.utils.validation import check_is_fitted

from .backend import is_device_array, is_sparse
from .base import BaseSom


class SomClassifier(BaseSom, TransformerMixin, ClassifierMixin):
    """Directed batch growing SOM classifier (see ``BaseSom`` for parameters)."""

    def _check_input_data(self, X, y):
        # (X's finite check rides on the device's column sums when it can; y is checked here as ever)
        # (missing_values="nan-fit": NaN passes in dense X -- BaseSom._check_fit_array)
        X, y = self._check_fit_array(X, y, supervised=True)
        X = self._check_sparse_input(X)
        return X, y

    def _label_prototypes(self, X, y) -> None:
        """Majority label and class frequencies of every prototype's Voronoi set
        (SomClassifier.py:130-152); a dead prototype gets label -1."""
        winners = self._resident_winners(X)
        m, n_classes = len(self.neurons_), self.classes_.shape[0]
        hits = self._node_stats["hit_count"]
        labels = np.empty(m, dtype=np.int64)
        probs = np.zeros((m, n_classes))
        sw = self._sw
        for j in range(m):
            if sw is not None:
                # rows of weight w count w times: weighted class counts; a tie goes to the tied class whose first
                # row of positive weight comes first (statistics.mode on the repeated rows)
                mask = (winners == j) & (sw > 0)
                members = y[mask]
                if len(members) == 0:
                    labels[j] = -1
                    probs[j, -1] = 0 / hits[j] if hits[j] > 0 else 1
                    continue
                counts = np.bincount(members, weights=sw[mask], minlength=n_classes)
                tied = np.flatnonzero(counts == counts.max())
                labels[j] = tied[0] if len(tied) == 1 else members[np.isin(members, tied).argmax()]
                ids = np.flatnonzero(counts)
                probs[j, ids] = counts[ids] / hits[j] if hits[j] > 0 else 1
                continue
            members = y[winners == j]
            if len(members) == 0:
                labels[j] = -1
                probs[j, -1] = 0 / hits[j] if hits[j] > 0 else 1
                continue
            labels[j] = mode(members)
            ids, counts = np.unique(members, return_counts=True)
            probs[j, ids] = counts / hits[j] if hits[j] > 0 else 1
        self._lattice.write_attributes({"label": labels, "probabilities": probs})

    def _refuse_vertical_device_query(self, X) -> None:
        if self.vertical_growth and is_device_array(X):
            raise ValueError("predict_proba / predict with vertical_growth=True walk the child maps row by row on the "
                             "host; " + self._HOST_ARRAY)

    def predict(self, X) -> np.ndarray:
        """The class of the largest probability.  A device array: the arg-max runs on its device and N indices
        come to the host (class labels need not be numbers: the result is a NumPy array)."""
        check_is_fitted(self)
        self._refuse_vertical_device_query(X)
        X = self._check_query(X)
        if is_device_array(X):
            return self.classes_[self._host(self.predict_proba(X=X).argmax(1))]
        return self.classes_[np.argmax(self.predict_proba(X=X), axis=1)]

    def predict_proba(self, X) -> np.ndarray:
        """Class probabilities: sparse code over the prototypes times the prototypes' class
        frequencies, rows normalised (SomClassifier.py:178-220)."""
        check_is_fitted(self)
        self._refuse_vertical_device_query(X)
        X = self._check_query(X)
        if self.vertical_growth:
            if self._accepts_nan() and isinstance(X, np.ndarray) and np.isnan(X).any():
                raise ValueError("predict_proba with vertical_growth=True takes complete rows only (impute them first)")
            _, winners = self._get_winning_neurons(X, n_bmu=1)
            rows = []
            for i, w in enumerate(winners):
                sample = X[i].toarray()[0] if is_sparse(X) else X[i]
                attrs = self.som_.nodes[self.neurons_[w]]
                if "som" in attrs:
                    # (a child map knows the classes of its Voronoi set only, by this map's class CODES --
                    #  what _grow_vertical hands it as y: back into this map's columns)
                    child = attrs["som"]
                    row = np.zeros(self.classes_.shape[0])
                    row[np.asarray(child.classes_, dtype=np.int64)] = child.predict_proba(sample[None, :])[0]
                    rows.append(row)
                else:
                    rows.append(attrs["probabilities"])
            return np.array(rows)
        # the code never leaves the backend: it returns (code @ P) normalised per row
        X = self._complete_query(X)
        return self._sparse_code(X, P=self._extract_values_from_graph("probabilities"))
