"""CPU: prototype_distances -- the oracle matrix against the search's own oracle, the shape tables against the
launcher they claim to cover, the estimator plumbing on a CPU stand-in backend, and the argument errors of the new
ABI calls as status codes."""
import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd.backend import HotPathBackend
from oracle import som_oracle as o
from tests import device_abi as da
from tests import golden_inputs as gi
from tests import prototype_distances as pd
from tests.test_missing_cpu import masked_distances, punch


# ---- the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pd.CASES, ids=pd.CASE_IDS)
def test_oracle_matrix_agrees_with_the_search_oracle(case):
    X, W, D = pd.case_data(case)
    Xw = da.widen(X)
    assert D.shape == (X.shape[0], W.shape[0]) and D.dtype == np.float64 and not np.isnan(D).any()
    d1, i1 = o.bmu_chain(Xw, W, 1)
    rows = np.arange(len(D))
    assert np.array_equal(D[rows, i1], d1) and np.array_equal(D.min(axis=1), d1)
    # no two different r share one square root at the minimum here: the arg-min of the matrix is the search's
    # (ties between duplicated prototypes go to the lowest index on both sides)
    assert np.array_equal(D.argmin(axis=1), i1)
    if W.shape[0] >= 2:
        d2, i2 = o.bmu_chain(Xw, W, 2)
        assert np.array_equal(np.take_along_axis(D, i2, axis=1), d2)
        order = np.argsort(D, axis=1, kind="stable")[:, :2]
        assert np.array_equal(np.take_along_axis(D, order, axis=1), d2) and np.array_equal(order, i2)
    if W.shape[0] >= 3:
        assert np.array_equal(D[:, 0], D[:, -1])                     # the duplicated prototype
        assert D[X.shape[0] // 2, W.shape[0] // 2] == 0.0            # the row that is a prototype


def test_oracle_matrix_rows_with_holes():
    X, _ = gi.blobs_f32(40, 6, 5, n_centers=3)
    W = np.random.default_rng(0).normal(size=(7, 6))
    Xn = punch(X, 0.4, 9)
    Xn[::3] = X[::3]
    holes = np.isnan(Xn).any(axis=1)
    D = pd.pair_distances(Xn, W)
    assert np.array_equal(D[holes], masked_distances(Xn[holes], W))
    assert np.array_equal(D[~holes], pd.pair_distances(Xn[~holes], W))


# ---- the tables -------------------------------------------------------------------------------------------------------
def test_tables_reach_every_launcher_form():
    forms = {(c[0],) + pd.launcher_form(c)[0] for c in pd.CASES}
    assert {("f32", "dma", 1), ("f32", "dma", 2), ("f32", "dma", 4), ("f64", "dma", 1), ("f64", "dma", 2),
            ("f32", "reg"), ("f64", "reg"), ("bf16", "reg")} <= forms
    for dtype in ("f32", "f64", "bf16"):                             # both store widths per storage type
        assert {pd.launcher_form(c)[1] for c in pd.CASES if c[0] == dtype} == {True, False}
    assert set(pd.N_VALUES) <= {c[1] for c in pd.CASES}
    assert set(pd.M_VALUES) <= {c[2] for c in pd.CASES}
    assert set(pd.D_VALUES) <= {c[3] for c in pd.CASES}
    assert {0, 3} <= {c[4] for c in pd.CASES} and 1 in {c[5] for c in pd.CASES}
    assert {c[6] for c in pd.CASES} == {0, 3} and {c[7] for c in pd.CASES} == {0, 1}
    # the DMA form with strided rows, and d % 16 == 0 that falls back to the register-staged form for its stride
    assert any(pd.launcher_form(c)[0][0] == "dma" and c[4] for c in pd.CASES)
    assert any(pd.launcher_form(c)[0][0] == "reg" and c[3] % 16 == 0 and c[0] != "bf16" for c in pd.CASES)
    # more than one sweep chunk in either form, and a second workgroup
    assert any(pd.launcher_form(c)[0][0] == "dma" and c[2] > 32 * pd.launcher_form(c)[0][1] for c in pd.CASES)
    assert any(pd.launcher_form(c)[0][0] == "reg" and c[2] > 128 for c in pd.CASES)
    assert any(c[1] > 128 for c in pd.CASES)


# ---- estimator plumbing on the stand-in ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=pd.DistancesOracleBackend(), missing_values="nan", random_state=0, n_iter=15,
                max_neurons=20).fit(X)
    return est, X


def test_shape_dtype_and_prototype_order(fitted):
    est, X = fitted
    D = est.prototype_distances(X[:90])
    assert isinstance(D, np.ndarray) and D.shape == (90, len(est.neurons_)) and D.dtype == np.float64
    assert np.array_equal(D, pd.pair_distances(X[:90], est.weights_))
    for j in (0, len(est.weights_) - 1):
        assert np.array_equal(D[:, j], o.bmu_chain(X[:90], est.weights_[j:j + 1], 1)[0])
    dist, idx = est._get_winning_neurons(X[:90], 1)
    assert np.array_equal(D.min(axis=1), dist) and np.array_equal(D[np.arange(90), idx], dist)
    assert np.array_equal(D[np.arange(90), est.predict(X[:90])], dist)
    assert est.calculate_quantization_error(X[:90]) == float(np.mean(D.min(axis=1)))
    # anything but float32 becomes float64, as for predict
    Xi = np.rint(X[:20]).astype(np.int64)
    assert np.array_equal(est.prototype_distances(Xi), pd.pair_distances(Xi.astype(np.float64), est.weights_))
    assert np.array_equal(est.prototype_distances(X[:20].tolist()),
                          pd.pair_distances(X[:20].astype(np.float64), est.weights_))


def test_classifier_inherits_it():
    X, y = gi.blobs_f32(300, 5, 4, n_centers=3)
    clf = SomClassifier(backend=pd.DistancesOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    D = clf.prototype_distances(X[:30])
    assert D.shape == (30, len(clf.neurons_)) and np.array_equal(D, pd.pair_distances(X[:30], clf.weights_))


def test_not_fitted_and_feature_mismatch(fitted):
    est, X = fitted
    with pytest.raises(NotFittedError):
        SomVQ(backend=pd.DistancesOracleBackend()).prototype_distances(X)
    with pytest.raises(ValueError, match="features"):
        est.prototype_distances(X[:10, :5])
    with pytest.raises(ValueError, match="features"):
        est.prototype_distances(sp.csr_matrix(X[:10, :5]))
    with pytest.raises(ValueError, match="features"):
        est.prototype_distances(np.empty((0, 3)))


def test_nan_is_refused_without_missing_values(fitted):
    est, X = fitted
    plain = SomVQ(backend=pd.DistancesOracleBackend(), random_state=0, n_iter=15, max_neurons=20).fit(X)
    Xn = punch(X[:40], 0.3, 3)
    with pytest.raises(ValueError, match="NaN"):
        plain.prototype_distances(Xn)
    with pytest.raises(ValueError, match="no observed entry"):
        est.prototype_distances(np.vstack([Xn, np.full((1, X.shape[1]), np.nan, dtype=X.dtype)]))
    with pytest.raises(ValueError, match="[Ii]nf"):
        est.prototype_distances(np.where(np.isnan(Xn), np.inf, Xn))
    assert np.array_equal(plain.prototype_distances(X[:40]), est.prototype_distances(X[:40]))


def test_split_and_scatter(fitted):
    est, X = fitted
    be = est._engine()
    Xn = punch(X[:200], 0.3, 2)
    Xn[::3] = X[:200:3]                                   # every third row complete
    incomplete = np.isnan(Xn).any(axis=1)
    be.distance_rows, be.masked_distance_rows = [], []
    D = est.prototype_distances(Xn)
    assert be.masked_distance_rows == [int(incomplete.sum())] and be.distance_rows == [int((~incomplete).sum())]
    assert np.array_equal(D[incomplete], masked_distances(Xn[incomplete], est.weights_))
    assert np.array_equal(D[~incomplete], pd.pair_distances(Xn[~incomplete], est.weights_))
    dist, idx = est._get_winning_neurons(Xn, 1)
    assert np.array_equal(D.min(axis=1), dist) and np.array_equal(D[np.arange(200), idx], dist)
    # no incomplete row: no masked call; nothing but incomplete rows: no dense call
    be.distance_rows, be.masked_distance_rows = [], []
    est.prototype_distances(X[:50])
    assert be.masked_distance_rows == [] and be.distance_rows == [50]
    be.distance_rows, be.masked_distance_rows = [], []
    est.prototype_distances(Xn[incomplete])
    assert be.masked_distance_rows == [int(incomplete.sum())] and be.distance_rows == []


def test_sparse_equals_dense(fitted):
    est, X = fitted
    Xs = np.where(np.abs(X[:120]) < 2.0, 0.0, X[:120]).astype(np.float32)
    want = est.prototype_distances(Xs)
    for fmt in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        assert np.array_equal(est.prototype_distances(fmt(Xs)), want)
    with pytest.raises(ValueError):                       # a NaN among the stored entries of sparse X: refused as ever
        bad = sp.csr_matrix(Xs)
        bad.data[0] = np.nan
        est.prototype_distances(bad)


def test_empty_input(fitted):
    est, X = fitted
    be = est._engine()
    be.distance_rows, be.masked_distance_rows = [], []
    for empty in (X[:0], np.empty((0, X.shape[1]))):
        D = est.prototype_distances(empty)
        assert isinstance(D, np.ndarray) and D.shape == (0, len(est.neurons_)) and D.dtype == np.float64
    assert be.distance_rows == [] and be.masked_distance_rows == []


def test_no_new_constructor_parameter():
    import inspect

    for cls in (SomVQ, SomClassifier):
        params = [p for p in inspect.signature(cls.__init__).parameters if p != "self"]
        assert params[-1] == "missing_values"             # still the last one
        assert list(cls().get_params()) == sorted(params)
        assert not [p for p in params if "chunk" in p or "prototype_dist" in p]


def test_base_backend_has_no_distance_matrix():
    with pytest.raises(NotImplementedError):
        HotPathBackend().distances(np.zeros((2, 3)), np.zeros((4, 3)))
    with pytest.raises(NotImplementedError):
        HotPathBackend().distances_masked(np.zeros((2, 3)), np.zeros((4, 3)))


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()   # noqa: E731
    one = 8                                 # any non-null address: argument errors come before any device work
    dist = lambda dt=0, N=10, d=4, ldx=4, M=5, ldo=5, p=one: lib.dbgsom_distances(   # noqa: E731
        p, dt, N, d, ldx, p, p, M, p, p, ldo, None)
    assert dist(dt=7) == -1 and b"x_dtype" in err()
    assert dist(ldo=4) == -1 and b"ldo" in err()
    assert dist(M=0, ldo=0) == -1 and b"M" in err()
    assert dist(M=_native.MAX_PROTOTYPES + 1, ldo=_native.MAX_PROTOTYPES + 1) == -1 and b"MAX_PROTOTYPES" in err()
    assert dist(ldx=3) == -1 and b"shape" in err()
    assert dist(p=None) == -1 and b"null pointer" in err()
    assert dist(N=0, p=None) == 0           # no rows: nothing to do, nothing dereferenced

    ws_need = lib.dbgsom_bmu_masked_workspace_bytes(0, 10, 4, 5)
    masked = lambda dt=0, N=10, d=4, ldx=4, M=5, ldw=4, ldo=5, p=one, ws=ws_need: lib.dbgsom_distances_masked(   # noqa: E731
        p, dt, N, d, ldx, p, M, ldw, p, ldo, p, ws, None)
    assert masked(dt=2) == -1 and b"x_dtype" in err()          # no bfloat16 rows with holes, as for the search
    assert masked(ldo=4) == -1 and b"ldo" in err()
    assert masked(M=0, ldo=0) == -1 and b"M" in err()
    assert masked(M=_native.MAX_PROTOTYPES + 1, ldo=_native.MAX_PROTOTYPES + 1) == -1 and b"MAX_PROTOTYPES" in err()
    assert masked(ldw=3) == -1 and b"ldw" in err()
    assert masked(p=None) == -1 and b"null pointer" in err()
    assert masked(ws=ws_need - 1) == -3 and b"workspace" in err()
    assert masked(N=0, p=None, ws=0) == 0

    W = np.zeros((5, 4))
    for name, args in (("dbgsom_ctx_distances_query", (None, one, 0, 10, 4, W.ctypes.data, 5, one)),
                       ("dbgsom_ctx_distances_query_device", (None, one, 0, 10, 4, 4, W.ctypes.data, 5, one, 5)),
                       ("dbgsom_ctx_distances_query_csr", (None, one, one, one, 0, 10, 4, 3, W.ctypes.data, 5, one)),
                       ("dbgsom_ctx_distances_query_masked", (None, one, 0, 10, 4, W.ctypes.data, 5, one))):
        assert getattr(lib, name)(*args) == -1 and b"null context" in err()
        with pytest.raises(ValueError, match="null context"):
            _native.call(name, *args)
