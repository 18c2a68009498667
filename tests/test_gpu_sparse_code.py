"""Sparse coding on the MI355X (csrc/sparse_code.hip): BaseSom.transform, SomClassifier.predict_proba
and predict against scikit-learn's SparseCoder computed here, on the golden maps and on shapes that
drive every branch of the LARS-lasso path (drops, degenerate regressors, the overflow pass).

Gates (DESIGN.md "Sparse coding"): max |dcode| <= 1e-10 for float64 queries, <= 1e-6 for float32
queries, predict_proba rtol 1e-9, predict labels identical."""
import warnings

import numpy as np
import pytest

from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu


def _sk_code(W, X):
    from sklearn.decomposition import SparseCoder
    from sklearn.preprocessing import normalize

    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    coder = SparseCoder(dictionary=normalize(W), positive_code=True, transform_alpha=0,
                        transform_algorithm="lasso_lars")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return coder.transform(normalize(X))


@pytest.fixture(scope="module")
def hip():
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0)
    yield be
    be.release()


def _map(name):
    return np.asarray(gi.load(name)["final_weights"], dtype=np.float64)


def _check(hip, W, X, tol, **kw):
    got = hip.sparse_code(W, X, **kw)
    ref = _sk_code(W, X)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= tol, f"max |dcode| = {err:.3e}"
    return got


@pytest.mark.parametrize("name", ["digits_clf", "digits_entropy"])
def test_transform_golden_maps_f64(hip, name):
    X, _ = gi.case_X(name)
    _check(hip, _map(name), X.astype(np.float64), 1e-10)


def test_drops_are_exercised(hip):
    X, _ = gi.case_X("digits_clf")
    _check(hip, _map("digits_clf"), X.astype(np.float64), 1e-10)
    assert hip.sparse_code_counts["drops"] > 0
    assert hip.sparse_code_counts["samples"] == X.shape[0]
    # several prototypes dropped in one step (exactly equal z) never happens on the golden map
    # (such steps are counted because they are handled one drop at a time)
    assert hip.sparse_code_counts["multi_drops"] == 0


def test_transform_f32_queries(hip):
    X, _ = gi.case_X("digits_f32")
    assert X.dtype == np.float32
    _check(hip, _map("digits_f32"), X, 1e-6)


def test_transform_blobs_dead_and_int_input(hip):
    X, _ = gi.case_X("blobs_dead")
    _check(hip, _map("blobs_dead"), X, 1e-10 if X.dtype == np.float64 else 1e-6)
    Xi, _ = gi.case_X("ties_int")
    Xi = np.asarray(Xi).astype(np.int32)
    assert Xi.dtype == np.int32
    _check(hip, _map("ties_int"), Xi, 1e-10)  # the backend converts integer input to float64, as check_array


def test_c2_shaped_subset_and_wide_map(hip):
    rng = np.random.default_rng(5)
    X, _ = gi.blobs_f32(2000, 784, 11)
    W = X[rng.choice(2000, 506, replace=False)].astype(np.float64) + rng.normal(0, 0.1, (506, 784))
    _check(hip, W, X, 1e-6)
    # M > d
    X16 = rng.normal(size=(300, 16))
    W16 = rng.normal(size=(64, 16))
    _check(hip, W16, X16, 1e-10)


def test_degenerate_regressors_warn(hip):
    """Exact copies of five prototypes send rows through the degenerate-regressor branch.  There the
    path is decided by rounding noise: scikit-learn against itself with G and Cov perturbed by 1e-15
    moves codes by up to 0.95 on these rows (DESIGN.md "Sparse coding", parity rule), so this case
    checks the branch's counters, the warning and a valid code, not the sklearn values."""
    from sklearn.exceptions import ConvergenceWarning

    W = _map("digits_clf")
    W = np.vstack([W, W[:5]])
    X, _ = gi.case_X("digits_clf")
    X = X[:400].astype(np.float64)
    with pytest.warns(ConvergenceWarning):
        got = hip.sparse_code(W, X)
    assert hip.sparse_code_counts["degenerate"] > 0
    assert got.shape == (400, W.shape[0]) and np.isfinite(got).all()


def test_overflow_pass_and_chunking_give_identical_results(hip):
    X, _ = gi.case_X("digits_clf")
    X = X.astype(np.float64)
    W = _map("digits_clf")
    base = hip.sparse_code(W, X)
    assert hip.sparse_code_counts["overflow"] == 0
    try:
        hip.sc_cap = 3
        capped = hip.sparse_code(W, X)
        assert hip.sparse_code_counts["overflow"] > 0
        assert np.array_equal(capped, base)
    finally:
        hip.sc_cap = 0
    old = hip.sc_chunk_rows
    try:
        hip.sc_chunk_rows = 250
        assert np.array_equal(hip.sparse_code(W, X), base)
    finally:
        hip.sc_chunk_rows = old


def test_zero_rows_and_empty_query(hip):
    W = _map("digits_clf")
    X, _ = gi.case_X("digits_clf")
    X = X[:10].astype(np.float64).copy()
    X[3] = 0.0
    code = hip.sparse_code(W, X)
    assert np.all(code[3] == 0.0)
    P = np.abs(np.random.default_rng(0).normal(size=(W.shape[0], 4)))
    pr = hip.sparse_code(W, X, P=P)
    assert np.all(np.isnan(pr[3])) and not np.isnan(pr[[0, 1, 2, 4]]).any()
    assert hip.sparse_code(W, X[:0]).shape == (0, W.shape[0])


@pytest.fixture(scope="module")
def fitted_clf():
    from dbgsom_amd import SomClassifier

    X, y = gi.case_X("digits_clf")
    est = SomClassifier(**gi.EST_KWARGS["digits_clf"]).fit(X, y)
    return est, X, y


def test_classifier_predict_proba_predict_score(fitted_clf):
    est, X, y = fitted_clf
    g = gi.load("digits_clf")
    P = est._extract_values_from_graph("probabilities")
    raw = _sk_code(est.weights_, X) @ P
    host = raw / raw.sum(axis=1)[:, None]
    np.testing.assert_allclose(est.predict_proba(X), host, rtol=1e-9, atol=1e-12)
    assert np.array_equal(est.predict(X), g["final_predict"])
    assert est.score(X, y) == float(g["final_score"])
    Xz = X[:5].astype(np.float64).copy()
    Xz[2] = 0.0
    assert est.predict(Xz)[2] == est.classes_[0]


def test_gpu_path_does_not_use_sparse_coder(fitted_clf, monkeypatch):
    """Fails without the feature: the estimator's transform / predict_proba must not reach sklearn."""
    est, X, _ = fitted_clf
    P = est._extract_values_from_graph("probabilities")
    ref_code = _sk_code(est.weights_, X)
    raw = ref_code @ P
    ref_proba = raw / raw.sum(axis=1)[:, None]

    import sklearn.decomposition

    class _Boom:
        def __init__(self, *a, **k):
            raise AssertionError("SparseCoder called on the GPU path")

    monkeypatch.setattr(sklearn.decomposition, "SparseCoder", _Boom)
    assert np.abs(est.transform(X) - ref_code).max() <= 1e-10
    np.testing.assert_allclose(est.predict_proba(X), ref_proba, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_norm_rows_follow_sklearn_normalize(hip, dtype):
    """sklearn's normalize leaves a row whose norm is below 10 eps of its dtype as it is
    (_handle_zeros_in_scale): its code and class probabilities must follow."""
    W = _map("digits_clf")
    X, _ = gi.case_X("digits_clf")
    X = X[:8].astype(dtype).copy()
    eps = np.finfo(dtype).eps
    X[1] = X[1] / np.linalg.norm(X[1].astype(np.float64)) * 2.0 * eps   # below the threshold
    X[2] = X[2] / np.linalg.norm(X[2].astype(np.float64)) * 50.0 * eps  # above it
    X[3] = 0.0
    X[3, 5] = dtype(1e-7 if dtype == np.float32 else 1e-16)
    tol = 1e-6 if dtype == np.float32 else 1e-10
    _check(hip, W, X, tol)
    P = np.abs(np.random.default_rng(1).normal(size=(W.shape[0], 3)))
    raw = _sk_code(W, X) @ P
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = raw / raw.sum(axis=1)[:, None]
    np.testing.assert_allclose(hip.sparse_code(W, X, P=P), ref, rtol=1e-9 if dtype == np.float64 else 1e-5,
                               atol=1e-12)


@pytest.mark.parametrize("d", [64, 13])
def test_resident_prototypes(d):
    """W = RESIDENT: the prototypes already in HBM (rows padded to a multiple of 16 features)."""
    from dbgsom_amd.backend import RESIDENT, HipBackend

    X, _ = gi.case_X("digits_clf")
    X = np.ascontiguousarray(X[:, :d], dtype=np.float64)
    W = X[np.random.default_rng(2).choice(X.shape[0], 40, replace=False)] + 0.25
    be = HipBackend(0)
    try:
        be.load(X)
        be.set_weights(W)
        got = be.sparse_code(RESIDENT, X[:300])
        assert np.array_equal(got, be.sparse_code(W, X[:300]))
        assert np.abs(got - _sk_code(W, X[:300])).max() <= 1e-10
    finally:
        be.release()
