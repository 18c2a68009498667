"""CPU: the host side of ``fit(X, y, sample_weight=w)`` -- validation, start prototypes, growing threshold,
total variance, the weighted majority label, dead-by-weight neurons -- against NumPy / an unweighted fit on
``np.repeat(X, w, axis=0)``, with a CPU stand-in backend (the oracle's, its per-neuron sums weighted)."""
from statistics import mode

import numpy as np
import pytest

from dbgsom_amd import SomClassifier, SomVQ
from oracle import som_oracle as o


class WeightedOracleBackend(o.OracleBackend):
    """OracleBackend whose epoch sums honour ``set_sample_weight``: S = sum w h x, K = sum w h, a = sum w,
    E = sum w dist over the rows of positive weight (TESTS ONLY, like its base class)."""

    def _local_sums(self, W, gamma, want_assignments):
        dist, win = self._fn(self._X, np.asarray(W), 1)
        sums = self._sums_from(W, o.exp_similarity_gamma(dist, gamma), win, dist)
        return sums, (win if want_assignments else None), (dist if want_assignments else None)

    def _sums_from(self, W, sample_weights, winners, distances):
        if self._sw is None:
            return super()._sums_from(W, sample_weights, winners, distances)
        M, keep, w = np.asarray(W).shape[0], self._sw > 0, self._sw
        S, K, _, E = o.accumulate(self._X[keep], winners[keep], (w * sample_weights)[keep], (w * distances)[keep], M)
        return self._pack(S, K, np.bincount(winners, weights=w, minlength=M), E)


def _digits():
    from sklearn.datasets import load_digits

    dg = load_digits()
    return dg.data[:900], dg.target[:900], np.random.default_rng(7).integers(0, 4, 900)


def test_fit_validates_sample_weight():
    X, y, w = _digits()
    est = SomVQ(random_state=0, n_iter=3, backend=WeightedOracleBackend())
    with pytest.raises(ValueError):
        est.fit(X, sample_weight=np.ones(899))                      # one weight per row
    with pytest.raises(ValueError):
        est.fit(X, sample_weight=np.ones((900, 2)))
    with pytest.raises(ValueError):
        est.fit(X, sample_weight=np.r_[-1.0, np.ones(899)])         # negative
    with pytest.raises(ValueError):
        est.fit(X, sample_weight=np.r_[np.nan, np.ones(899)])       # NaN
    with pytest.raises(ValueError, match="all zero"):
        est.fit(X, sample_weight=np.zeros(900))
    few = np.zeros(900)
    few[[3, 50, 700]] = 2.0
    with pytest.raises(ValueError, match="minimum of 4"):
        est.fit(X, sample_weight=few)                               # fewer than 4 rows of positive weight
    with pytest.raises(ValueError):
        SomClassifier(random_state=0, n_iter=3, backend=WeightedOracleBackend()).fit(X, y, sample_weight=-np.ones(900))
    few[10] = 0.5
    est.fit(X, sample_weight=few)                                   # four rows: accepted, scalar weights too
    est.fit(X, sample_weight=2.0)
    assert np.array_equal(est.fit_predict(X, sample_weight=w), est.fit(X, sample_weight=w).labels_)
    assert est.fit_transform(X, sample_weight=w).shape == (900, len(est.neurons_))


def test_host_side_of_a_weighted_fit_equals_numpy_on_repeated_rows():
    """the figures of the issue: 223 rows of weight 0, sum w = 1401, start rows 238, 457, 772, 574"""
    X, _, w = _digits()
    Xr = np.repeat(X, w, axis=0)
    assert (w == 0).sum() == 223 and w.sum() == 1401
    est = SomVQ(random_state=0, n_iter=40, backend=WeightedOracleBackend())
    est._engine().load(X)
    est._load_resident(X)
    est._attach_sample_weight(X, est._check_sample_weight(w, X))
    rows = est._draw_weighted_rows(np.random.default_rng(0))
    assert rows.tolist() == [238, 457, 772, 574]
    assert np.array_equal(X[rows], np.random.default_rng(0).choice(a=Xr, size=4, replace=False))
    est._initialize_som(X)
    assert np.array_equal(est.weights_, np.random.default_rng(0).choice(a=Xr, size=4, replace=False))
    np.testing.assert_allclose(est._total_variance, np.var(Xr, axis=0).sum(), rtol=1e-12)
    np.testing.assert_allclose(est.growing_threshold_,
                               150 * -np.log(0.5) * np.linalg.norm(np.std(Xr, axis=0, ddof=1)), rtol=1e-12)
    np.testing.assert_allclose(est._total_variance, 1185.8693571075214, rtol=1e-12)
    np.testing.assert_allclose(est.growing_threshold_, 3581.7081358491637, rtol=1e-12)


def test_weighted_fit_equals_the_fit_on_repeated_rows():
    X, y, w = _digits()
    Xr, yr = np.repeat(X, w, axis=0), np.repeat(y, w)
    a = SomVQ(random_state=0, n_iter=40, backend=WeightedOracleBackend()).fit(X, sample_weight=w)
    b = SomVQ(random_state=0, n_iter=40, backend=o.OracleBackend()).fit(Xr)
    assert a.neurons_ == b.neurons_ and a.n_iter_ == b.n_iter_ and len(a.neurons_) == 18
    np.testing.assert_allclose(a.weights_, b.weights_, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(a.quantization_error_, b.quantization_error_, rtol=1e-12)
    np.testing.assert_allclose(a.quantization_error_, 24.603818810781167, rtol=1e-12)
    np.testing.assert_allclose(a.topographic_error_, 0.07351891506067094, rtol=1e-12)
    assert np.array_equal(np.repeat(a.labels_, w), b.labels_)
    assert np.array_equal(a._extract_values_from_graph("hit_count"), b._extract_values_from_graph("hit_count"))
    np.testing.assert_allclose(a._extract_values_from_graph("density"), b._extract_values_from_graph("density"), rtol=1e-10)
    for kw in (dict(n_iter=30), dict(n_iter=30, growth_criterion="entropy", spreading_factor=0.4, max_neurons=40)):
        c = SomClassifier(random_state=0, backend=WeightedOracleBackend(), **kw).fit(X, y, sample_weight=w)
        r = SomClassifier(random_state=0, backend=o.OracleBackend(), **kw).fit(Xr, yr)
        assert c.neurons_ == r.neurons_ and c.n_iter_ == r.n_iter_
        np.testing.assert_allclose(c.weights_, r.weights_, rtol=1e-10, atol=1e-12)
        assert np.array_equal(c._extract_values_from_graph("label"), r._extract_values_from_graph("label"))
        np.testing.assert_allclose(c._extract_values_from_graph("probabilities"),
                                   r._extract_values_from_graph("probabilities"), rtol=1e-12, atol=1e-15)


def test_weighted_majority_label_breaks_ties_like_mode_on_repeated_rows():
    """one neuron, class counts tied at 3 : 3 : 1 by weight: the tied class whose first row of positive weight comes first"""
    rng = np.random.default_rng(0)
    X = rng.normal(size=(8, 3))
    y = np.array([2, 1, 0, 2, 1, 0, 1, 2])
    w = np.array([0.0, 1.0, 1.0, 3.0, 1.0, 0.0, 1.0, 0.0])          # class 2: 3 (first positive row 3), class 1: 3 (row 1)
    est = SomClassifier(random_state=0, n_iter=2, backend=WeightedOracleBackend())
    est.fit(X, y, sample_weight=w)
    est._sw = w
    winners = np.zeros(8, dtype=np.int64)
    est._get_winning_neurons = lambda data, n_bmu: (np.zeros(8), winners)
    est._node_stats = {"hit_count": np.full(len(est.neurons_), w.sum())}
    est._label_prototypes(X, y)
    lab = est._extract_values_from_graph("label")
    assert lab[0] == mode(np.repeat(y, w.astype(int))) == 1
    np.testing.assert_allclose(est._extract_values_from_graph("probabilities")[0], [1 / 7, 3 / 7, 3 / 7])
    assert np.all(lab[1:] == -1)


def test_neurons_whose_rows_all_have_weight_zero_are_removed():
    rng = np.random.default_rng(3)
    X = np.r_[rng.normal(size=(300, 4)), rng.normal(size=(40, 4)) + 30.0]   # a far cluster ...
    w = np.r_[np.ones(300), np.zeros(40)]                                   # ... that does not count
    a = SomVQ(random_state=1, n_iter=20, backend=WeightedOracleBackend()).fit(X, sample_weight=w)
    b = SomVQ(random_state=1, n_iter=20, backend=o.OracleBackend()).fit(X[:300])
    assert a.neurons_ == b.neurons_
    np.testing.assert_allclose(a.weights_, b.weights_, rtol=1e-10, atol=1e-12)
    assert np.all(a._extract_values_from_graph("hit_count") > 0)
    assert np.all(np.abs(a.weights_).max(axis=1) < 15)                      # no prototype went to the far cluster


def test_all_ones_weights_are_the_unweighted_start_and_scalars_exactly():
    X, _, _ = _digits()
    a = SomVQ(random_state=0, n_iter=12, backend=o.OracleBackend()).fit(X)
    b = SomVQ(random_state=0, n_iter=12, backend=WeightedOracleBackend()).fit(X, sample_weight=np.ones(900))
    for est, sw in ((SomVQ(random_state=0, backend=o.OracleBackend()), None),
                    (SomVQ(random_state=0, backend=WeightedOracleBackend()), np.ones(900))):
        est._engine().load(X)
        est._load_resident(X)
        est._attach_sample_weight(X, est._check_sample_weight(sw, X))
        est._initialize_som(X)
        if sw is None:
            first = est
    assert np.array_equal(first.weights_, est.weights_)                      # the same four start rows
    assert first.growing_threshold_ == est.growing_threshold_ and first._total_variance == est._total_variance
    assert a.growing_threshold_ == b.growing_threshold_
    assert a.neurons_ == b.neurons_ and a.n_iter_ == b.n_iter_
    np.testing.assert_allclose(a.weights_, b.weights_, rtol=1e-10, atol=1e-12)
    assert a.topographic_error_ == b.topographic_error_


def test_a_backend_does_not_keep_the_weights_of_an_earlier_fit():
    X, _, w = _digits()
    be = WeightedOracleBackend()
    SomVQ(random_state=0, n_iter=8, backend=be).fit(X, sample_weight=w)
    assert be._sw is None
    be._sw = w.astype(np.float64)                                   # (left behind by a caller of its own)
    a = SomVQ(random_state=0, n_iter=8, backend=be).fit(X)
    b = SomVQ(random_state=0, n_iter=8, backend=o.OracleBackend()).fit(X)
    assert a.quantization_error_ == b.quantization_error_ and a.topographic_error_ == b.topographic_error_
    assert np.array_equal(a._extract_values_from_graph("hit_count"), b._extract_values_from_graph("hit_count"))
