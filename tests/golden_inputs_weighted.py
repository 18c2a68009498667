"""Inputs of the weighted golden cases (``fit(X, y, sample_weight=w)``), regenerated from seeds.  The
fixtures tests/golden/weighted_*.npz hold what the REFERENCE computed on ``np.repeat(X, w, axis=0)``
(tools/make_golden.py, section "weighted"): for integer weights that is, term by term, the weighted fit."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FIT_CASES = ["weighted_digits_vq", "weighted_digits_clf", "weighted_digits_entropy"]
CLF_CASES = ("weighted_digits_clf", "weighted_digits_entropy")
VERTICAL_CASE = "weighted_vertical_blobs"

EST_KWARGS = {
    "weighted_digits_vq": dict(random_state=0, n_iter=40),
    "weighted_digits_clf": dict(random_state=0, n_iter=40),
    "weighted_digits_entropy": dict(random_state=0, n_iter=30, growth_criterion="entropy",
                                    spreading_factor=0.4, max_neurons=40),
    "weighted_vertical_blobs": dict(random_state=2, vertical_growth=True, n_iter=24, max_neurons=9,
                                    min_samples_vertical_growth=150, spreading_factor=0.6),
}


def load(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def case(name):
    """-> (X, y or None, w): the distinct rows, their labels and their integer weights (some are 0)"""
    if name in FIT_CASES:
        from sklearn.datasets import load_digits

        dg = load_digits()
        w = np.random.default_rng(7).integers(0, 4, 900)
        return dg.data[:900], (dg.target[:900] if name in CLF_CASES else None), w
    if name == VERTICAL_CASE:
        from sklearn.datasets import make_blobs

        X = make_blobs(n_samples=4000, n_features=10, centers=7, cluster_std=2.0, random_state=4)[0]
        return X, None, np.random.default_rng(7).integers(0, 4, 4000)
    raise KeyError(name)


def repeated(name):
    """-> (np.repeat(X, w, 0), np.repeat(y, w) or None): what the reference was run on"""
    X, y, w = case(name)
    return np.repeat(X, w, axis=0), (None if y is None else np.repeat(y, w))
