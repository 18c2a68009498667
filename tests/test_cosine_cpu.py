"""CPU: ``metric="cosine"`` -- the fma emulation against exact rationals, the emulated chain against the pinned oracle,
the restatement of the contract against extended precision and scikit-learn, its edge values, the estimator plumbing on
a CPU stand-in backend (a case where the metrics disagree, invariants of the queries, every refusal, the other metrics
untouched), a whole fit on angular blobs, the argument errors of the new calls as status codes, and the coverage of the
shape table the GPU tests run."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.base import clone
from sklearn.metrics.pairwise import cosine_distances as sk_cosine_distances

from dbgsom_amd import SomClassifier, SomVQ, _native
from oracle import som_oracle as o
from tests import cosine as cs
from tests import device_abi as da
from tests import manhattan as mh
from tests import prototype_distances as pd


# ---- 1. the oracle ------------------------------------------------------------------------------------------------
def test_fma_emulation_against_exact_rationals():
    rng = np.random.default_rng(3)
    n = 4000
    x = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)
    w = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)
    acc = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)
    near = slice(0, n // 2)                                                    # near-cancellation: acc ~ -x w
    acc[near] = -(x[near] * w[near]) * (1.0 + rng.integers(-4, 5, n // 2) * 2.0 ** -52)
    got = cs.fma_exact(x, w, acc)
    plain_differs = 0
    for i in range(n):
        exact = Fraction(float(x[i])) * Fraction(float(w[i])) + Fraction(float(acc[i]))
        want = float(exact)                                                    # (Fraction -> float rounds to nearest even)
        assert got[i] == want, (i, x[i], w[i], acc[i])
        plain_differs += (x[i] * w[i] + acc[i]) != want
    assert plain_differs > n // 10                                             # the plain multiply-add is not the fma


def test_plain_form_needs_float32_operands():
    X = np.array([[0.1, 0.2]])
    with pytest.raises(AssertionError):
        cs.dot_chain(X, X, exact=False)
    X32 = X.astype(np.float32)
    assert np.array_equal(cs.dot_chain(X32, X32.astype(np.float64), exact=False), cs.dot_chain(X32, X32.astype(np.float64), exact=True))


@pytest.mark.parametrize("N,M,d", [(6, 5, 50), (17, 9, 3), (5, 3, 1), (4, 7, 129)])
def test_emulated_chain_against_the_pinned_oracle(N, M, d):
    """sqrt(max((q + -2 a) + p, 0)) of the emulated chains is oracle/bmu_chain.c bit for bit: same a, q and p"""
    rng = np.random.default_rng(N + M + d)
    X = rng.normal(size=(N, d)) * 10.0 ** rng.uniform(-1, 1, (N, d))
    W = rng.normal(size=(M, d)) * 10.0 ** rng.uniform(-1, 1, (M, d))
    a, q, p = cs.dot_chain(X, W, exact=True), cs.sqnorm_chain(X, exact=True), cs.sqnorm_chain(W, exact=True)
    assert np.array_equal(q, o.row_sqnorms_chain(X)) and np.array_equal(p, o.row_sqnorms_chain(W))
    r = (q[:, None] + (-2.0 * a)) + p[None, :]
    assert np.array_equal(np.sqrt(np.maximum(r, 0.0)), pd.pair_distances(X, W))
    X32 = X.astype(np.float32)                                                 # ... and the plain form where it applies
    W32 = W.astype(np.float32).astype(np.float64)
    assert np.array_equal(cs.dot_chain(X32, W32, exact=False), cs.dot_chain(X32, W32, exact=True))


@pytest.mark.parametrize("kind", cs.RESTATEMENT_KINDS)
@pytest.mark.parametrize("d", cs.RESTATEMENT_D)
def test_restatement_against_extended_precision_and_sklearn(d, kind):
    assert da.have_longdouble()                                                # (x87 extended precision: 64-bit significand)
    X, W = cs.restatement_data(kind, d)
    C = cs.cosine_distances(X, W)
    bound = cs.error_bound(d)
    ref = cs.cosine_longdouble(X, W)
    ref = np.clip(ref, 0, 2)
    err_l = float(np.max(np.abs(C.astype(np.longdouble) - ref)))
    err_s = float(np.max(np.abs(C - sk_cosine_distances(np.asarray(X, dtype=np.float64), W))))
    print(f"d={d} {kind}: {err_l / bound:.3f} of the bound against longdouble, {err_s / bound:.3f} against scikit-learn")
    assert err_l <= bound
    assert err_s <= 2 * bound
    assert (C >= 0).all() and (C <= 2).all()


def test_edge_values():
    W = np.array([[1.0, 2.0, 2.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -2.0], [0.3, 0.1, -0.7]])
    X = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [0.3, 0.1, -0.7], [np.nan, 1.0, 1.0], [np.inf, 1.0, 1.0],
                  [1e200, 1.0, 1.0], [1e-200, 0.0, 0.0]])
    C = cs.cosine_distances(X, W)
    assert C[0].tolist() == [1.0, 1.0, 1.0, 1.0]                               # a zero row: 1 from everything
    assert C[1:3, 1].tolist() == [1.0, 1.0]                                    # a zero prototype
    assert C[1, 0] == 0.0 and C[1, 2] == 2.0                                   # equal (3 * (1/3) * (1/3) * 3: exact), opposite
    assert 0.0 <= C[2, 3] <= 2 * cs.U                                          # equal, after the clamp
    assert C[6].tolist() == [1.0, 1.0, 1.0, 1.0]                               # the squared norm underflows to 0
    assert np.isnan(C[3:6]).all()
    for k in (1, 2):
        dist, idx = cs.select(C, k)
        assert (idx[3:6] == -1).all() and np.isinf(dist[3:6]).all()
        assert idx[0].tolist() == [0, 1][:k]                                   # ties: the lowest index
    assert cs.inv_norms([0.0, 4.0, np.inf, np.nan, -1.0, 5e-324])[[0, 1]].tolist() == [0.0, 0.5]
    assert np.isnan(cs.inv_norms([np.inf, np.nan, -1.0])).all() and np.isfinite(cs.inv_norms([5e-324])).all()


# ---- 2. must fail without the feature -----------------------------------------------------------------------------
def _fitted_on(W, metric, cls=SomVQ):
    """an estimator whose map is W (no fit: the attributes a query reads)"""
    est = cls(backend=cs.CosineOracleBackend(), metric=metric)
    est.weights_ = np.asarray(W, dtype=np.float64)
    est.n_features_in_ = est.weights_.shape[1]
    est.neurons_ = [(i, 0) for i in range(len(W))]
    return est


def test_the_cosine_winner_is_not_the_euclidean_one():
    W = np.array([[1.0, 0.2], [9.0, 5.0]])
    X = np.array([[10.0, 0.0]])
    est = _fitted_on(W, "cosine")
    assert est.predict(X).tolist() == [0]                                      # the angle of (1, 0.2) is the smaller one
    C = cs.cosine_distances(X, W)
    assert C[0, 0] < C[0, 1] and np.array_equal(est.prototype_distances(X), C)
    dist, idx = est.kneighbors(X, n_neighbors=2)
    assert idx.tolist() == [[0, 1]] and np.array_equal(dist, C)
    assert est.calculate_quantization_error(X) == C[0, 0]
    for name in ("euclidean", "chebyshev", "manhattan"):
        assert _fitted_on(W, name, SomVQ).set_params(backend=mh.ManhattanOracleBackend()).predict(X).tolist() == [1]


@pytest.fixture(scope="module")
def fitted():
    X, lab = cs.angular_blobs()
    est = SomVQ(backend=cs.CosineOracleBackend(), metric="cosine", **cs.FIT_KW).fit(X)
    return est, X, lab


def test_a_fit_on_angular_blobs_grows_under_the_metric(fitted):
    est, X, _ = fitted
    be = est._engine()
    assert be.cosine_epochs >= 1 and be.euclidean_epochs == 0
    assert be._metric == "euclidean"                                           # given back after the fit
    assert np.isfinite(est.weights_).all() and len(est.weights_) > 4           # the map grew past its start neurons


# ---- 3. estimator plumbing ------------------------------------------------------------------------------------------
def test_fit_results_are_cosine_results(fitted):
    est, X, _ = fitted
    C = cs.cosine_distances(X, est.weights_)
    assert np.array_equal(est.labels_, np.argmin(C, axis=1))
    assert np.array_equal(est.predict(X), est.labels_)
    seen = est._engine().reduced_on
    Cq = cs.cosine_distances(X, seen["quantization_error"])
    assert est.quantization_error_ == pytest.approx(float(np.mean(Cq.min(axis=1))), rel=1e-15)
    Wt, pos = seen["topographic_error"]
    two = np.argsort(cs.cosine_distances(X, Wt), axis=1, kind="stable")[:, :2]
    assert est.topographic_error_ == np.count_nonzero(np.linalg.norm(pos[two[:, 0]] - pos[two[:, 1]], axis=1) > 1.5) / len(X)
    assert est.calculate_quantization_error(X) == pytest.approx(float(np.mean(C.min(axis=1))), rel=1e-15)
    pos = np.asarray(est.neurons_, dtype=np.float64)
    two = np.argsort(C, axis=1, kind="stable")[:, :2]
    apart = np.linalg.norm(pos[two[:, 0]] - pos[two[:, 1]], axis=1) > 1.5
    assert est._calculate_topographic_error(X) == np.count_nonzero(apart) / len(X)


def test_query_invariants(fitted):
    est, X, _ = fitted
    Q = X[:50].astype(np.float64) * 1.5 + 0.05
    C = est.prototype_distances(Q)
    assert np.array_equal(C, cs.cosine_distances(Q, est.weights_))
    k = min(5, len(est.weights_))
    dist, idx = est.kneighbors(Q, n_neighbors=k)
    assert np.array_equal(idx[:, 0], est.predict(Q))
    assert np.array_equal(dist, np.take_along_axis(C, idx, axis=1))
    assert np.array_equal(C.min(axis=1), dist[:, 0])
    assert est.calculate_quantization_error(Q) == pytest.approx(float(np.mean(C.min(axis=1))), rel=1e-15)
    assert np.array_equal(est.kneighbors(Q, n_neighbors=k, return_distance=False), idx)
    assert est.transform(Q).shape == (50, len(est.weights_))                   # the sparse code has no metric


def test_classifier_fit(fitted):
    _, X, lab = fitted
    be = cs.CosineOracleBackend()
    clf = SomClassifier(backend=be, metric="cosine", **cs.FIT_KW).fit(X, lab)
    assert be.cosine_epochs >= 1 and be.euclidean_epochs == 0
    win = np.argmin(cs.cosine_distances(X, clf.weights_), axis=1)
    labels = np.array([clf.som_.nodes[n]["label"] for n in clf.neurons_])
    for j in np.unique(win):                                                   # majority label of the cosine Voronoi set
        counts = np.bincount(lab[win == j], minlength=cs.N_CLASSES)
        assert counts[labels[j]] == counts.max()
    pred = clf.predict(X[:50])
    assert pred.shape == (50,) and set(pred) <= set(np.unique(lab))


def test_refusals_name_the_metric(fitted):
    est, X, _ = fitted
    new = lambda **kw: SomVQ(backend=cs.CosineOracleBackend(), metric="cosine", n_iter=3, **kw)
    with pytest.raises(ValueError, match="cosine.*sparse.*toarray"):
        new().fit(sp.csr_matrix(X))
    with pytest.raises(ValueError, match="cosine.*sparse.*toarray"):
        est.predict(sp.csr_matrix(X[:5]))
    holes = np.array(X)
    holes[3, 1] = np.nan
    with pytest.raises(ValueError, match="cosine.*missing entries.*impute"):
        new(missing_values="nan-fit").fit(holes)
    q = clone(est).set_params(missing_values="nan")
    q.weights_, q.n_features_in_, q.neurons_ = est.weights_, est.n_features_in_, est.neurons_
    for call in (q.predict, q.prototype_distances, lambda a: q.kneighbors(a, 2), q.calculate_quantization_error):
        with pytest.raises(ValueError, match="cosine.*missing entries"):
            call(holes[:8])
    assert np.array_equal(q.predict(X[:8]), est.predict(X[:8]))                # complete rows pass under missing_values
    with pytest.raises(ValueError, match="cosine.*sample_weight.*repeat"):
        new().fit(X, sample_weight=np.ones(len(X)))
    with pytest.raises(ValueError, match="cosine.*vertical_growth"):
        new(vertical_growth=True).fit(X)
    with pytest.raises(ValueError, match="cosine.*sharded_input"):
        new(sharded_input=True).fit(X)
    with pytest.raises(ValueError, match="cosine.*topographic_function"):
        est.topographic_function(X)
    with pytest.raises(ValueError, match="metric must be a string"):
        SomVQ(backend=cs.CosineOracleBackend(), metric=1, n_iter=3).fit(X)
    with pytest.raises(NotImplementedError):                                   # no quiet fall-back on a backend without it
        SomVQ(backend=o.OracleBackend(), metric="cosine", random_state=0, n_iter=3).fit(X)
    with pytest.raises(ValueError, match="'euclidean', 'manhattan' or 'cosine'"):
        cs.CosineOracleBackend().set_metric("chebyshev")


def test_other_metrics_are_unchanged(fitted):
    _, X, _ = fitted
    kw = dict(cs.FIT_KW)
    a = SomVQ(backend=o.OracleBackend(), metric="euclidean", **kw).fit(X)
    b = SomVQ(backend=o.OracleBackend(), metric="chebyshev", **kw).fit(X)
    assert np.array_equal(a.weights_, b.weights_) and np.array_equal(a.labels_, b.labels_)
    be = cs.CosineOracleBackend()
    c = SomVQ(backend=be, metric="euclidean", **kw).fit(X)
    assert be.cosine_epochs == 0 and be.cosine_queries == 0 and be.euclidean_epochs >= 1
    assert np.array_equal(c.weights_, a.weights_)
    SomVQ(backend=be, metric="cosine", **kw).fit(X)                            # the backend object serves a Euclidean fit afterwards
    after = SomVQ(backend=be, metric="euclidean", **kw).fit(X)
    assert np.array_equal(after.weights_, a.weights_) and np.array_equal(after.labels_, a.labels_)
    mb = mh.ManhattanOracleBackend()
    m = SomVQ(backend=mb, metric="manhattan", **kw).fit(X)
    assert mb.manhattan_epochs >= 1 and mb.euclidean_epochs == 0
    assert np.array_equal(m.labels_, np.argmin(mh.l1_distances(X, m.weights_), axis=1))


# ---- 4. the new calls: argument errors are status codes, before any launch ----------------------------------------
def test_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()
    assert lib.dbgsom_inv_norms(None, -1, None, None) == -1 and b"bad n" in err()
    assert lib.dbgsom_inv_norms(None, 0, None, None) == 0
    assert lib.dbgsom_inv_norms(None, 5, 8, None) == -1 and b"null pointer" in err()
    assert lib.dbgsom_inv_norms(12, 5, 8, None) == -1 and b"aligned" in err()
    bmu = lambda *a: lib.dbgsom_bmu_cosine(*a)
    assert bmu(None, 2, 10, 4, 4, None, None, 5, None, 1, None, None, None) == -1 and b"DBGSOM_F32 or DBGSOM_F64" in err()
    assert bmu(None, 0, 10, 4, 4, None, None, 5, None, 3, None, None, None) == -1 and b"k must be 1 or 2" in err()
    assert bmu(None, 0, 10, 4, 3, None, None, 5, None, 1, None, None, None) == -1 and b"bad sample shape" in err()
    assert bmu(None, 0, 10, 4, 4, None, None, 1, None, 2, None, None, None) == -1 and b"k <= M" in err()
    assert bmu(None, 0, 10, 4, 4, None, None, 5, None, 1, None, None, None) == -1 and b"null pointer" in err()
    assert bmu(None, 0, 0, 4, 4, None, None, 5, None, 1, None, None, None) == 0                   # no rows
    dist = lambda *a: lib.dbgsom_distances_cosine(*a)
    assert dist(None, 2, 10, 4, 4, None, None, 5, None, None, 5, None) == -1 and b"DBGSOM_F32 or DBGSOM_F64" in err()
    assert dist(None, 0, 10, 4, 4, None, None, 5, None, None, 4, None) == -1 and b"ldo" in err()
    assert dist(None, 0, 10, 4, 4, None, None, da.MAX_PROTOTYPES + 1, None, None, da.MAX_PROTOTYPES + 1, None) == -1
    assert dist(8, 0, 10, 4, 4, 8, 8, 5, 8, 12, 5, None) == -1 and b"8-byte aligned" in err()
    assert lib.dbgsom_kneighbors_cosine_workspace_bytes(100, 9, 0) == lib.dbgsom_kneighbors_workspace_bytes(100, 9, 0)
    knn = lambda *a: lib.dbgsom_kneighbors_cosine(*a)
    assert knn(None, 2, 10, 4, 4, None, None, 5, None, 2, 0, None, None, None, 0, None) == -1 and b"x_dtype" in err()
    assert knn(None, 0, 10, 4, 4, None, None, 5, None, 6, 0, None, None, None, 0, None) == -1 and b"k <= M" in err()
    assert knn(None, 0, 10, 4, 4, None, None, 50, None, 33, 0, None, None, None, 0, None) == -1 and b"DBGSOM_MAX_NEIGHBORS" in err()
    assert knn(None, 0, 10, 4, 4, None, None, 5, None, 2, -1, None, None, None, 0, None) == -1 and b"slab_rows" in err()
    rc = knn(16, 0, 10, 4, 4, 16, 16, 5, 16, 2, 0, 16, 16, 16, 16, None)
    need = lib.dbgsom_kneighbors_cosine_workspace_bytes(10, 5, 0)
    assert rc == -3 and b"workspace of 16 bytes" in err() and str(need).encode() in err()       # both sizes
    ctx_args = {"dbgsom_ctx_bmu_cosine": (None, None, 5, 1, None, None),
                "dbgsom_ctx_epoch_cosine": (None, None, 5, 0.1, 1.0, 0, None, None, None, None, None, None),
                "dbgsom_ctx_bmu_query_cosine": (None, None, 0, 10, 4, None, 5, 1, None, None),
                "dbgsom_ctx_bmu_query_cosine_device": (None, None, 0, 10, 4, 4, None, 5, 1, None, None),
                "dbgsom_ctx_distances_query_cosine": (None, None, 0, 10, 4, None, 5, None),
                "dbgsom_ctx_distances_query_cosine_device": (None, None, 0, 10, 4, 4, None, 5, None, 5),
                "dbgsom_ctx_kneighbors_query_cosine": (None, None, 0, 10, 4, None, 5, 1, None, None),
                "dbgsom_ctx_kneighbors_query_cosine_device": (None, None, 0, 10, 4, 4, None, 5, 1, None, None)}
    for name, args in ctx_args.items():
        assert getattr(lib, name)(*args) == -1 and b"null context" in err(), name


# ---- 5. the table the GPU tests run -----------------------------------------------------------------------------------
def test_the_shape_table_reaches_every_launcher_form():
    assert all(c[0] in ("f32", "f64") for c in cs.CASES) and len(cs.CASES) == len(pd.CASES) - 5
    forms = {(c[0],) + cs.launcher_form(c)[0] for c in cs.CASES}
    assert {("f32", "dma", 1), ("f32", "dma", 2), ("f32", "dma", 4), ("f64", "dma", 1), ("f64", "dma", 2),
            ("f32", "reg"), ("f64", "reg")} <= forms
    for dtype in ("f32", "f64"):                                               # 16-byte and 8-byte stores, both kernels
        for kind in ("dma", "reg"):
            assert {cs.launcher_form(c)[1] for c in cs.CASES if c[0] == dtype and cs.launcher_form(c)[0][0] == kind} == {True, False}
    assert {c[1] for c in cs.CASES} == set(pd.N_VALUES) and {c[2] for c in cs.CASES} == set(pd.M_VALUES)
    assert {c[3] for c in cs.CASES} >= set(pd.D_VALUES)
    X, W, C = cs.case_data(cs.CASES[0])                                         # the ties of a table entry
    assert (C[0] == 1.0).all() and np.array_equal(C[:, 0], C[:, -1])
