"""CPU: BaseSom.topographic_function / phi through the host default of the backend (the oracle's
k = 2 search + unweighted shortest paths) against the reference's own results on the golden maps
(tests/golden/topofn.npz, tools/make_golden_topofn.py).  Equality is exact: every value is an
integer count divided by M."""
import copy
import pickle

import numpy as np
import pytest
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ
from oracle.som_oracle import OracleBackend
from tests import golden_inputs as gi

# fixture case -> (golden fit case, estimator class)
CASES = {
    "digits_f64": ("digits_f64", SomVQ),
    "digits_f32": ("digits_f32", SomVQ),
    "digits_clf": ("digits_clf", SomClassifier),
    "grow_blobs_f32": ("grow_blobs_f32", SomVQ),
    "blobs_dead": ("blobs_dead", SomVQ),
    "ties_int": ("ties_int", SomVQ),
    "digits_few": ("digits_f64", SomVQ),
}


def golden():
    return gi.load("topofn")


def fitted(case, backend):
    """An estimator holding the golden map of `case` as its fitted state (no fit needed)."""
    fit_case, cls = CASES[case]
    g = gi.load(fit_case)
    est = cls(backend=backend)
    est.weights_ = np.asarray(g["final_weights"])
    est.neurons_ = [tuple(int(v) for v in p) for p in g["final_neurons"]]
    est.n_features_in_ = est.weights_.shape[1]
    X, _ = gi.case_X(fit_case)
    return est, X[: int(golden()[f"{case}_nq"])]


def check_against_golden(est, case, k_pos, k_neg):
    g = golden()
    assert k_pos.dtype == np.float64 and k_neg.dtype == np.float64
    assert np.array_equal(k_pos, g[f"{case}_k_pos"])
    assert np.array_equal(k_neg, g[f"{case}_k_neg"])
    got = np.array([est.phi(int(k)) for k in g[f"{case}_phi_k"]], dtype=np.int64)
    assert np.array_equal(got, g[f"{case}_phi"])


@pytest.mark.parametrize("case", list(CASES))
def test_matches_reference(case):
    est, X = fitted(case, OracleBackend())
    k_pos, k_neg = est.topographic_function(X)
    check_against_golden(est, case, k_pos, k_neg)


def test_digits_sanity_values():
    est, X = fitted("digits_f64", OracleBackend())
    k_pos, k_neg = est.topographic_function(X)
    assert np.array_equal(k_pos, [2.88, 2.8, 1.52, 0.48, 0.08])
    assert np.array_equal(k_neg, [2.88, 0.08, 0, 0, 0])
    assert [est.phi(k) for k in (-1, 0, 1, 2, 50, -30)] == [2, 72, 70, 38, 0, 0]


@pytest.mark.parametrize("case", ["grow_blobs_f32", "blobs_dead", "digits_few"])
def test_host_distances_match_reference(case):
    est, X = fitted(case, OracleBackend())
    hp, hn, D = est._engine().topographic_function(est.weights_, X, est.neurons_, want_distances=True)
    assert D.dtype == np.int32
    assert np.array_equal(D, golden()[f"{case}_D"])
    # histogram mode gives the same histograms
    hp2, hn2, none = est._engine().topographic_function(est.weights_, X, est.neurons_)
    assert none is None and np.array_equal(hp, hp2) and np.array_equal(hn, hn2)
    assert hn.sum() % 2 == 0 and hp.sum() % 2 == 0  # ordered pairs


def test_phi_before_call_raises_attribute_error():
    est, _ = fitted("digits_f64", OracleBackend())
    with pytest.raises(AttributeError):
        est.phi(1)


def test_unfitted_raises():
    X, _ = gi.case_X("digits_f64")
    with pytest.raises(NotFittedError):
        SomVQ(backend=OracleBackend()).topographic_function(X)


def test_feature_mismatch_raises():
    est, X = fitted("digits_f64", OracleBackend())
    with pytest.raises(ValueError, match="features"):
        est.topographic_function(X[:, :10])


def test_single_neuron_raises():
    est, X = fitted("digits_f64", OracleBackend())
    est.weights_ = est.weights_[:1]
    est.neurons_ = est.neurons_[:1]
    with pytest.raises(ValueError, match="n_neighbors"):
        est.topographic_function(X)


def test_pickle_and_copy_keep_phi():
    est, X = fitted("blobs_dead", OracleBackend())
    est.topographic_function(X)
    g = golden()
    ks = [int(k) for k in g["blobs_dead_phi_k"]]
    want = [est.phi(k) for k in ks]
    for other in (pickle.loads(pickle.dumps(est)), copy.deepcopy(est)):
        assert [other.phi(k) for k in ks] == want
    # the stored state is two small integer histograms, not dense M x M matrices
    for name in ("euclid_dist_matrix", "manhattan_dist_matrix", "max_dist_matrix", "_delaunay_maxtrix"):
        assert not hasattr(est, name)
