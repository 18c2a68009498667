"""CPU: ``metric="manhattan"`` -- the NumPy restatement of the L1 chain against scikit-learn, the (dist, index)
selection against argmin / a stable argsort, the estimator plumbing on a CPU stand-in backend (fits, invariants of the
queries, every refusal, the Euclidean path untouched), and the argument errors of the new device-level calls as status
codes."""
import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.base import clone
from sklearn.metrics.pairwise import manhattan_distances

from dbgsom_amd import SomClassifier, SomVQ, _native
from oracle import som_oracle as o
from tests import manhattan as mh


# ---- 1. the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("N,d,M", mh.SKLEARN_SHAPES)
def test_oracle_against_sklearn(N, d, M, dtype):
    rng = np.random.default_rng(N + d + M)
    X = rng.normal(size=(N, d)).astype(mh.NP_DTYPE[dtype])
    W = rng.normal(size=(M, d))
    got = mh.l1_distances(X, W)
    want = manhattan_distances(X.astype(np.float64), W)
    same = np.array_equal(got, want)
    print(f"bit for bit: {same}; largest relative difference {np.max(np.abs(got - want) / want):.3e}")
    if not same:   # (another summation order in scikit-learn: both are within (d + 1) u of the exact sum)
        assert np.all(np.abs(got - want) <= mh.l1_error_bound(X, W) * want)
    exact = np.array([[sum(abs(float(x) - float(w)) for x, w in zip(xr, wr)) for wr in W] for xr in X[:3].astype(np.float64)])
    assert np.all(np.abs(got[:3] - exact) <= mh.l1_error_bound(X, W) * exact)


def test_oracle_is_the_literal_chain():
    X, W = mh.raw_case("f32", 5, 7, 3)
    D = mh.l1_distances(X, W)
    for i in range(5):
        for j in range(3):
            acc = 0.0
            for k in range(7):
                acc = acc + abs(float(X[i, k]) - float(W[j, k]))
            assert acc == D[i, j]
    assert mh.l1_distances(W, W).diagonal().tolist() == [0.0, 0.0, 0.0]     # exact zero for a row equal to a prototype


def test_selection_against_argmin_and_stable_argsort():
    rng = np.random.default_rng(5)
    D = rng.integers(0, 6, (40, 9)).astype(np.float64)                        # many ties
    d1, i1 = mh.l1_select(D, 1)
    assert np.array_equal(i1[:, 0], np.argmin(D, axis=1)) and np.array_equal(d1[:, 0], D.min(axis=1))
    for k in (2, 5, 9):
        dk, ik = mh.l1_select(D, k)
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        assert np.array_equal(ik, order) and np.array_equal(dk, np.take_along_axis(D, order, axis=1))
    D[3] = np.nan
    D[4, :] = np.inf
    D[5, 2:] = np.inf
    dk, ik = mh.l1_select(D, 3)
    assert ik[3].tolist() == [-1, -1, -1] and ik[4].tolist() == [-1, -1, -1] and np.isinf(dk[3]).all()
    assert ik[5].tolist()[2] == -1 and set(ik[5].tolist()[:2]) == {0, 1}


# ---- 2. must fail without the feature -----------------------------------------------------------------------------
def _fitted_on(W, metric, cls=SomVQ):
    """an estimator whose map is W (no fit: the attributes a query reads)"""
    est = cls(backend=mh.ManhattanOracleBackend(), metric=metric)
    est.weights_ = np.asarray(W, dtype=np.float64)
    est.n_features_in_ = est.weights_.shape[1]
    est.neurons_ = [(i, 0) for i in range(len(W))]
    return est


def test_the_l1_winner_is_not_the_euclidean_one():
    W = np.array([[3.0, 0.0], [2.0, 2.0]])
    X = np.array([[0.0, 0.0]])
    for name in ("manhattan", "cityblock", "l1"):
        est = _fitted_on(W, name)
        assert est.predict(X).tolist() == [0]                                 # |3| + |0| = 3 < |2| + |2| = 4
        assert est.prototype_distances(X).tolist() == [[3.0, 4.0]]
        dist, idx = est.kneighbors(X, n_neighbors=2)
        assert idx.tolist() == [[0, 1]] and dist.tolist() == [[3.0, 4.0]]
        assert est.calculate_quantization_error(X) == 3.0
    for name in ("euclidean", "chebyshev"):
        assert _fitted_on(W, name).predict(X).tolist() == [1]                 # sqrt(8) < 3


@pytest.fixture(scope="module")
def fitted():
    X, lab = mh.blobs()
    be = mh.ManhattanOracleBackend()
    est = SomVQ(backend=be, metric="manhattan", **mh.FIT_KW).fit(X)
    return est, X, lab


def test_a_fit_under_the_metric_calls_epoch_manhattan(fitted):
    est, X, _ = fitted
    be = est._engine()
    assert be.manhattan_epochs >= 1 and be.euclidean_epochs == 0
    assert be._metric == "euclidean"                                          # given back after the fit
    assert np.isfinite(est.weights_).all() and len(est.weights_) >= 4


# ---- 3. estimator plumbing ------------------------------------------------------------------------------------------
def test_fit_results_are_l1_results(fitted):
    est, X, _ = fitted
    D = mh.l1_distances(X, est.weights_)
    assert np.array_equal(est.labels_, np.argmin(D, axis=1))
    assert np.array_equal(est.predict(X), est.labels_)
    # the statistics of the fit are taken on the resident rows under the prototypes of that moment (the snapshot the
    # last epoch consumed, dead neurons still in): the L1 values on those
    seen = est._engine().reduced_on
    Dq = mh.l1_distances(X, seen["quantization_error"])
    assert est.quantization_error_ == pytest.approx(float(np.mean(Dq.min(axis=1))), rel=1e-15)
    Wt, pos = seen["topographic_error"]
    two = np.argsort(mh.l1_distances(X, Wt), axis=1, kind="stable")[:, :2]
    assert est.topographic_error_ == np.count_nonzero(np.linalg.norm(pos[two[:, 0]] - pos[two[:, 1]], axis=1) > 1.5) / len(X)
    # ... and the same calls on the fitted map as queries
    assert est.calculate_quantization_error(X) == pytest.approx(float(np.mean(D.min(axis=1))), rel=1e-15)
    pos = np.asarray(est.neurons_, dtype=np.float64)
    two = np.argsort(D, axis=1, kind="stable")[:, :2]
    apart = np.linalg.norm(pos[two[:, 0]] - pos[two[:, 1]], axis=1) > 1.5
    assert est._calculate_topographic_error(X) == np.count_nonzero(apart) / len(X)


def test_query_invariants(fitted):
    est, X, _ = fitted
    Q = X[:50].astype(np.float64) + 0.25
    D = est.prototype_distances(Q)
    assert np.array_equal(D, mh.l1_distances(Q, est.weights_))
    k = min(5, len(est.weights_))
    dist, idx = est.kneighbors(Q, n_neighbors=k)
    assert np.array_equal(idx[:, 0], est.predict(Q))
    assert np.array_equal(dist, np.take_along_axis(D, idx, axis=1))
    assert np.array_equal(est.kneighbors(Q, n_neighbors=k, return_distance=False), idx)
    assert est.transform(Q).shape == (50, len(est.weights_))                  # the sparse code has no metric


def test_classifier_fit(fitted):
    _, X, lab = fitted
    be = mh.ManhattanOracleBackend()
    clf = SomClassifier(backend=be, metric="l1", **mh.FIT_KW).fit(X, lab)
    assert be.manhattan_epochs >= 1 and be.euclidean_epochs == 0
    win = np.argmin(mh.l1_distances(X, clf.weights_), axis=1)
    labels = np.array([clf.som_.nodes[n]["label"] for n in clf.neurons_])
    for j in np.unique(win):                                                  # majority label of the L1 Voronoi set
        counts = np.bincount(lab[win == j], minlength=mh.N_CLASSES)
        assert counts[labels[j]] == counts.max()
    pred = clf.predict(X[:50])                                                # (the sparse code: no metric in it)
    assert pred.shape == (50,) and set(pred) <= set(np.unique(lab))
    ent = SomClassifier(backend=mh.ManhattanOracleBackend(), metric="manhattan", growth_criterion="entropy",
                        **mh.FIT_KW).fit(X, lab)
    assert ent._engine().manhattan_epochs >= 1


def test_refusals_name_the_metric(fitted):
    est, X, _ = fitted
    new = lambda **kw: SomVQ(backend=mh.ManhattanOracleBackend(), metric="manhattan", n_iter=3, **kw)
    with pytest.raises(ValueError, match="manhattan.*sparse.*toarray"):
        new().fit(sp.csr_matrix(X))
    with pytest.raises(ValueError, match="manhattan.*sparse.*toarray"):
        est.predict(sp.csr_matrix(X[:5]))
    holes = np.array(X)
    holes[3, 1] = np.nan
    with pytest.raises(ValueError, match="manhattan.*missing entries.*impute"):
        new(missing_values="nan-fit").fit(holes)
    q = clone(est).set_params(missing_values="nan")
    q.weights_, q.n_features_in_, q.neurons_ = est.weights_, est.n_features_in_, est.neurons_
    for call in (q.predict, q.prototype_distances, lambda a: q.kneighbors(a, 2), q.calculate_quantization_error):
        with pytest.raises(ValueError, match="manhattan.*missing entries"):
            call(holes[:8])
    assert np.array_equal(q.predict(X[:8]), est.predict(X[:8]))               # complete rows pass under missing_values
    with pytest.raises(ValueError, match="manhattan.*sample_weight.*repeat"):
        new().fit(X, sample_weight=np.ones(len(X)))
    with pytest.raises(ValueError, match="manhattan.*vertical_growth"):
        new(vertical_growth=True).fit(X)
    with pytest.raises(ValueError, match="manhattan.*sharded_input"):
        new(sharded_input=True).fit(X)
    with pytest.raises(ValueError, match="manhattan.*topographic_function"):
        est.topographic_function(X)
    with pytest.raises(ValueError, match="metric must be a string"):
        SomVQ(backend=mh.ManhattanOracleBackend(), metric=1, n_iter=3).fit(X)


def test_wide_rows_far_from_every_prototype_are_refused_by_name():
    """gamma d^2 > 36.7 for every row of a neuron: its centre is 0 / 0, as in the reference's update; the fit says so"""
    rng = np.random.default_rng(0)
    X = (rng.normal(size=(300, 784)) + 3.0 * rng.integers(0, 8, (300, 1))).astype(np.float32)
    with pytest.raises(ValueError, match="manhattan.*not finite.*sample kernel.*reduce the features"):
        SomVQ(backend=mh.ManhattanOracleBackend(), metric="manhattan", random_state=0, n_iter=20).fit(X)
    est = SomVQ(backend=mh.ManhattanOracleBackend(), metric="manhattan", random_state=0, n_iter=8).fit(X[:, :16])
    assert np.isfinite(est.weights_).all()


def test_euclidean_and_unknown_strings_take_todays_path(fitted):
    _, X, _ = fitted
    fits = {}
    for name in ("euclidean", "chebyshev"):
        fits[name] = SomVQ(backend=o.OracleBackend(), metric=name, **mh.FIT_KW).fit(X)
    a, b = fits["euclidean"], fits["chebyshev"]
    assert np.array_equal(a.weights_, b.weights_) and np.array_equal(a.labels_, b.labels_)
    be = mh.ManhattanOracleBackend()
    c = SomVQ(backend=be, metric="euclidean", **mh.FIT_KW).fit(X)
    assert be.manhattan_epochs == 0 and be.manhattan_queries == 0 and be.euclidean_epochs >= 1
    assert np.array_equal(c.weights_, a.weights_)
    c.predict(X[:5])
    assert be.manhattan_queries == 0
    with pytest.raises(NotImplementedError):                                   # no quiet fall-back on a backend without it
        SomVQ(backend=o.OracleBackend(), metric="manhattan", random_state=0, n_iter=3).fit(X)


def test_the_backend_object_serves_a_euclidean_fit_afterwards(fitted):
    _, X, _ = fitted
    be = mh.ManhattanOracleBackend()
    before = SomVQ(backend=be, **mh.FIT_KW).fit(X)
    SomVQ(backend=be, metric="manhattan", **mh.FIT_KW).fit(X)
    after = SomVQ(backend=be, **mh.FIT_KW).fit(X)
    assert np.array_equal(before.weights_, after.weights_) and np.array_equal(before.labels_, after.labels_)


# ---- 4. the new device-level calls: argument errors are status codes, before any launch ---------------------------
def test_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()
    assert lib.dbgsom_bmu_manhattan_workspace_bytes(0, 0, 0, 0) == 0
    f32 = lib.dbgsom_bmu_manhattan_workspace_bytes(0, 100, 7, 9)
    f64 = lib.dbgsom_bmu_manhattan_workspace_bytes(1, 100, 7, 9)
    assert f64 >= 7 * 256 * 8 and f32 >= f64 + 100 * 7 * 8                     # Wt; float32 rows: their float64 copy too
    assert lib.dbgsom_kneighbors_manhattan_workspace_bytes(1, 100, 7, 9, 0) >= f64 + 100 * 10 * 8
    rc = lib.dbgsom_bmu_manhattan(None, 2, 10, 4, 4, None, 5, 4, 1, None, None, None, 0, None)
    assert rc == -1 and b"x_dtype" in err()                                    # no bfloat16 rows
    rc = lib.dbgsom_bmu_manhattan(None, 0, 10, 4, 4, None, 5, 4, 3, None, None, None, 0, None)
    assert rc == -1 and b"k must be 1 or 2" in err()
    rc = lib.dbgsom_bmu_manhattan(None, 0, 10, 4, 3, None, 5, 4, 1, None, None, None, 0, None)
    assert rc == -1 and b"bad sample shape" in err()                           # ldx < d
    rc = lib.dbgsom_bmu_manhattan(None, 0, 10, 4, 4, None, 5, 3, 1, None, None, None, 0, None)
    assert rc == -1 and b"ldw" in err()
    rc = lib.dbgsom_bmu_manhattan(None, 0, 10, 4, 4, None, 1, 4, 2, None, None, None, 0, None)
    assert rc == -1 and b"k <= M" in err()
    rc = lib.dbgsom_bmu_manhattan(None, 0, 10, 4, 4, None, 5, 4, 1, None, None, None, 0, None)
    assert rc == -1 and b"null pointer" in err()
    assert lib.dbgsom_bmu_manhattan(None, 0, 0, 4, 4, None, 5, 4, 1, None, None, None, 0, None) == 0    # no rows
    rc = lib.dbgsom_bmu_manhattan(8, 0, 10, 4, 4, 8, 5, 4, 1, 8, 8, 8, 16, None)
    need = lib.dbgsom_bmu_manhattan_workspace_bytes(0, 10, 4, 5)
    assert rc == -3 and b"workspace of 16 bytes" in err() and str(need).encode() in err()   # both sizes
    rc = lib.dbgsom_distances_manhattan(None, 0, 10, 4, 4, None, 5, 4, None, 4, None, 0, None)
    assert rc == -1 and b"ldo" in err()
    rc = lib.dbgsom_distances_manhattan(8, 1, 10, 4, 4, 8, 5, 4, 8, 5, 8, 16, None)
    assert rc == -3 and b"workspace of 16 bytes" in err()
    rc = lib.dbgsom_kneighbors_manhattan(None, 0, 10, 4, 4, None, 5, 4, 6, 0, None, None, None, 0, None)
    assert rc == -1 and b"k <= M" in err()                                     # M below k
    rc = lib.dbgsom_kneighbors_manhattan(None, 0, 10, 4, 4, None, 50, 4, 33, 0, None, None, None, 0, None)
    assert rc == -1 and b"DBGSOM_MAX_NEIGHBORS" in err()
    rc = lib.dbgsom_kneighbors_manhattan(None, 0, 10, 4, 4, None, 5, 4, 2, -1, None, None, None, 0, None)
    assert rc == -1 and b"slab_rows" in err()
    rc = lib.dbgsom_kneighbors_manhattan(8, 0, 10, 4, 4, 8, 5, 4, 2, 0, 8, 8, 8, 16, None)
    assert rc == -3 and b"workspace of 16 bytes" in err()
    for name in ("dbgsom_ctx_bmu_manhattan", "dbgsom_ctx_bmu_query_manhattan", "dbgsom_ctx_distances_query_manhattan",
                 "dbgsom_ctx_kneighbors_query_manhattan"):
        args = {"dbgsom_ctx_bmu_manhattan": (None, None, 5, 1, None, None),
                "dbgsom_ctx_bmu_query_manhattan": (None, None, 0, 10, 4, None, 5, 1, None, None),
                "dbgsom_ctx_distances_query_manhattan": (None, None, 0, 10, 4, None, 5, None),
                "dbgsom_ctx_kneighbors_query_manhattan": (None, None, 0, 10, 4, None, 5, 1, None, None)}[name]
        assert getattr(lib, name)(*args) == -1 and b"null context" in err()
