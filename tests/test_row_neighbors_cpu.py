"""CPU: index_rows / row_neighbors -- the restatement of rho against a long-double sum, the oracle against a plain sort,
the NumPy default of the backend (the statement of the semantics) against scikit-learn's brute-force search, the
invariants, every refusal of the estimator, the pickle round trip, and the argument errors of the C entries as status
codes (no GPU is touched: a null context is refused after the argument checks)."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd import backend as bk
from tests import golden_inputs as gi
from tests import row_neighbors as rn
from tests.test_device_input_cpu import FakeDeviceArray

KW = dict(random_state=0, n_iter=12)


# ---- rho_rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 127, 129, 784, 4097])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e6])
def test_rho_rows_within_the_bound_of_the_long_double_sum(d, dtype, scale):
    rng = np.random.default_rng(d)
    X = (rng.normal(size=(32, d)) * scale).astype(dtype)
    q = (rng.normal(size=d) * scale).astype(dtype)
    got = rn.rho_rows(X, q)
    t = X.astype(np.longdouble) - q.astype(np.longdouble)
    exact = (t * t).sum(axis=1)
    err = np.abs(got.astype(np.longdouble) - exact) / exact
    print("d=%d %s scale=%g: worst %.3f of the bound" % (d, np.dtype(dtype).name, scale, float(err.max() / rn.rho_bound(d))))
    assert (err <= rn.rho_bound(d)).all()
    assert np.array_equal(got.view(np.uint64), bk.rho_rows(X, q).view(np.uint64))     # the product's copy: the same bits


# ---- the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand,k", [(0, 3), (1, 3), (5, 5), (70, 1), (300, 32)])
def test_oracle_against_a_plain_sort_of_tuples(n_cand, k):
    case = rn.scan_case(n_cand + k, n_cand, 9, k, np.float64, np.float32)
    if n_cand >= 256:
        rn.plant_specials(case)
    a = rn.oracle(case["X"], case["winners"], case["probes"], case["Q"], k)
    b = rn.oracle_sorted_tuples(case["X"], case["winners"], case["probes"], case["Q"], k)
    c = bk.nearest_rows_host(case["X"], case["winners"], case["probes"], case["Q"], k)
    for other in (b, c):
        assert np.array_equal(a[1], other[1]) and np.array_equal(a[0].view(np.uint64), other[0].view(np.uint64))
    assert (a[1][0, min(k, n_cand):] == -1).all() and np.isinf(a[0][0, min(k, n_cand):]).all()


def test_buckets_of_the_table():
    winners = np.array([2, 0, 2, 5, 0, 2, 7, -1])
    order, seg = rn.buckets(winners, 6)
    assert list(seg) == [0, 2, 2, 5, 5, 5, 6] and list(order[:6]) == [1, 4, 0, 2, 5, 3]
    assert list(rn.buckets(winners, 6, descending=True)[0][:6]) == [4, 1, 5, 2, 0, 3]
    case = rn.scan_case(1, 257, 3, 2)
    assert case["seg"][2] - case["seg"][1] == 0                       # unit 1: an empty cell between full ones
    assert (case["seg"][1] - case["seg"][0]) + (case["seg"][3] - case["seg"][2]) == 257
    assert -1 in case["probes"][0]


# ---- the stand-in: estimator on the NumPy default -------------------------------------------------------------------
def _digits(n=600, dtype=np.float32):
    return np.ascontiguousarray(gi.case_X("digits_f64")[0][:n], dtype=dtype)


@pytest.fixture(scope="module", params=["vq", "clf"])
def indexed(request):
    X = _digits()
    be = rn.RowNeighborsOracleBackend()
    if request.param == "vq":
        est = SomVQ(backend=be, **KW).fit(X)
    else:
        est = SomClassifier(backend=be, **KW).fit(X, gi.case_X("digits_clf")[1][:600])
    before = {k: np.copy(v) for k, v in vars(est).items() if k.endswith("_") and isinstance(v, np.ndarray)}
    assert est.index_rows(X) is est
    for k, v in before.items():                                       # the map and what fit set stay as they are
        assert np.array_equal(getattr(est, k), v, equal_nan=True)
    return est, X


def test_index_attributes(indexed):
    est, X = indexed
    M = len(est.weights_)
    assert est.n_indexed_ == len(X)
    assert est.index_counts_.dtype == np.int64 and est.index_counts_.shape == (M,)
    assert np.array_equal(est.index_counts_, np.bincount(est.kneighbors(X, 1, return_distance=False)[:, 0], minlength=M))


def test_all_units_agree_with_brute_force(indexed):
    """n_probe = M: the exact search.  scikit-learn's brute-force NearestNeighbors is asked for the direct form
    (metric="seuclidean" with unit variances: sqrt(sum (x - y)^2 / 1), evaluated pair by pair), whose own error is
    below the bound.  Its default evaluates |x|^2 - 2 <x, y> + |y|^2, whose cancellation error on this data is 7.9
    times the bound on its own (measured against rho_rows, which lies within the bound of the exact sum) and says
    nothing about the code under test."""
    from sklearn.neighbors import NearestNeighbors

    est, X = indexed
    M = len(est.weights_)
    assert M <= 32
    Xu, first = np.unique(X, axis=0, return_index=True)               # data without duplicated rows
    est2 = pickle.loads(pickle.dumps(est))
    est2.backend = est2._backend_obj = rn.RowNeighborsOracleBackend()
    est2.index_rows(Xu)
    rng = np.random.default_rng(0)
    Q = (Xu[rng.choice(len(Xu), 30)] + rng.normal(size=(30, X.shape[1]))).astype(np.float32)
    dist, idx = est2.row_neighbors(Q, 10, M)
    nn = NearestNeighbors(n_neighbors=10, algorithm="brute", metric="seuclidean", metric_params=dict(V=np.ones(X.shape[1])))
    want = nn.fit(Xu.astype(np.float64)).kneighbors(Q.astype(np.float64))[0]
    t = Q.astype(np.longdouble)[:, None, :] - Xu.astype(np.longdouble)[idx]
    exact = np.sqrt((t * t).sum(axis=2))
    # against the exact distance of the listed row: half the bound on rho, and the root's rounding
    assert (np.abs(dist - exact) <= (rn.rho_bound(X.shape[1]) / 2 + rn.U) * exact).all()
    print("worst against scikit-learn: %.3f of the bound" % float(np.max(np.abs(dist - want) / want) / rn.rho_bound(X.shape[1])))
    assert (np.abs(dist - want) <= rn.rho_bound(X.shape[1]) * want).all()


def test_invariants(indexed):
    est, X = indexed
    M = len(est.weights_)
    rows = np.arange(0, len(X), 11)
    dist, idx = est.row_neighbors(X[rows], 5, min(3, M))
    assert dist.dtype == np.float64 and idx.dtype == np.int64 and dist.shape == idx.shape == (len(rows), 5)
    assert (dist[:, 0] == 0).all()
    assert all(np.array_equal(X[i], X[r]) and i <= r for i, r in zip(idx[:, 0], rows))
    assert np.array_equal(est.row_neighbors(X[rows], 5, min(3, M), return_distance=False), idx)
    units = est.kneighbors(X[rows], min(3, M), return_distance=False)
    unit_of = est.kneighbors(X, 1, return_distance=False)[:, 0]
    for q in range(len(rows)):
        assert np.isin(unit_of[idx[q][idx[q] >= 0]], units[q]).all()
    # a smaller n_probe lists a subset of the candidates: with every candidate listed (k = 32 on small cells) a subset
    small = est.row_neighbors(X[rows], 32, 1, return_distance=False)
    large = est.row_neighbors(X[rows], 32, min(3, M), return_distance=False)
    for q in range(len(rows)):
        a, b = small[q][small[q] >= 0], large[q][large[q] >= 0]
        if len(b) < 32:
            assert set(a) <= set(b)
    # (inf, -1) fill: a unit with fewer rows than k
    j = int(np.argmin(np.where(est.index_counts_ > 0, est.index_counts_, len(X))))
    q = X[unit_of == j][:1]
    d1, i1 = est.row_neighbors(q, 32, 1)
    n = min(32, int(est.index_counts_[j]))
    assert (i1[0, :n] >= 0).all() and (i1[0, n:] == -1).all() and np.isinf(d1[0, n:]).all()
    # no rows: no call
    d0, i0 = est.row_neighbors(np.empty((0, X.shape[1]), dtype=np.float32), 4)
    assert d0.shape == i0.shape == (0, 4)


def test_argument_errors_in_kneighbors_wording(indexed):
    est, X = indexed
    M = len(est.weights_)
    for kw in (dict(n_neighbors=2.0), dict(n_probe=True), dict(n_neighbors="3")):
        with pytest.raises(ValueError, match="does not take .* value, enter integer value"):
            est.row_neighbors(X[:2], **kw)
    with pytest.raises(ValueError, match="Expected n_neighbors > 0. Got 0"):
        est.row_neighbors(X[:2], 0)
    with pytest.raises(ValueError, match="Expected n_probe > 0. Got -1"):
        est.row_neighbors(X[:2], 3, -1)
    with pytest.raises(ValueError, match="n_neighbors = 33 is above the 32"):
        est.row_neighbors(X[:2], 33)
    with pytest.raises(ValueError, match="Expected n_probe <= n_samples_fit, but n_probe = %d" % (M + 1)):
        est.row_neighbors(X[:2], 3, M + 1)
    with pytest.raises(ValueError, match="features"):
        est.row_neighbors(X[:2, :5])


def test_refusals(indexed):
    est, X = indexed
    with pytest.raises(TypeError, match="dense rows"):
        est.row_neighbors(sp.csr_matrix(X[:3]))
    with pytest.raises(TypeError, match="dense rows"):
        est.index_rows(sp.csr_matrix(X))
    bad = X[:3].copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError):
        est.row_neighbors(bad)
    with pytest.raises(ValueError):
        est.index_rows(np.concatenate([bad, X[:5]]))
    other = FakeDeviceArray(X[:3].copy(), index=1)
    with pytest.raises(ValueError, match="GPU 1"):
        est.row_neighbors(other)
    with pytest.raises(ValueError, match="GPU 1"):
        est.index_rows(FakeDeviceArray(X.copy(), index=1))
    est.index_rows(X)                                                 # (the refused calls may have dropped the index)
    for name, value, pattern in (("metric", "manhattan", "Manhattan"), ("metric", "cosine", "cosine"),
                                 ("sharded_input", True, "one process")):
        old = getattr(est, name)
        setattr(est, name, value)
        try:
            with pytest.raises(ValueError, match=pattern):
                est.row_neighbors(X[:3])
            with pytest.raises(ValueError, match=pattern):
                est.index_rows(X)
        finally:
            setattr(est, name, old)
    old = est.missing_values
    est.missing_values = "nan"
    try:
        with pytest.raises(ValueError, match="missing entries"):
            est.row_neighbors(bad)
        with pytest.raises(ValueError, match="missing entries"):
            est.index_rows(np.concatenate([bad, X[:5]]))
    finally:
        est.missing_values = old
    est.index_rows(X)
    est.row_neighbors(X[:3])


def test_wide_rows_are_refused_by_name(indexed):
    est, X = indexed
    old = est.n_features_in_
    est.n_features_in_ = 8193
    try:
        with pytest.raises(ValueError, match="8192"):
            est.index_rows(np.zeros((4, 8193), dtype=np.float32))
        with pytest.raises(ValueError, match="8192"):
            est.row_neighbors(np.zeros((1, 8193), dtype=np.float32))
    finally:
        est.n_features_in_ = old


def test_no_index_pickle_fit_and_replaced_rows():
    X = _digits(300)
    est = SomVQ(backend=rn.RowNeighborsOracleBackend(), **KW).fit(X)
    with pytest.raises(ValueError, match="index_rows"):
        est.row_neighbors(X[:2], 2, 2)
    est.index_rows(X)
    dist, idx = est.row_neighbors(X[:7], 3, 2)
    other = pickle.loads(pickle.dumps(est))
    assert np.array_equal(other.index_counts_, est.index_counts_) and other.n_indexed_ == 300
    with pytest.raises(ValueError, match="index_rows"):
        other.row_neighbors(X[:2], 2, 2)
    other.backend = other._backend_obj = rn.RowNeighborsOracleBackend()
    other.index_rows(X)
    d2, i2 = other.row_neighbors(X[:7], 3, 2)
    assert np.array_equal(i2, idx) and np.array_equal(d2, dist)
    est._engine().load(X[:100])                                       # a call that replaced the resident rows
    with pytest.raises(ValueError, match="replaced"):
        est.row_neighbors(X[:2], 2, 2)
    est.index_rows(X)
    est.fit(X)
    with pytest.raises(ValueError, match="index_rows"):
        est.row_neighbors(X[:2], 2, 2)


def test_backend_default_needs_its_partition():
    X = _digits(200, np.float64)
    be = rn.RowNeighborsOracleBackend().load(X)
    W = X[:6] + 0.5
    with pytest.raises(ValueError, match="partition"):
        be.row_neighbors(W, 2, 2, X[:3])
    counts, win = be.partition(W, want_winners=True)
    assert counts.sum() == 200 and np.array_equal(counts, np.bincount(win, minlength=6))
    dist, idx = be.row_neighbors(W, 2, 6, X[:3])
    assert list(idx[:, 0]) == [0, 1, 2] and (dist[:, 0] == 0).all()
    with pytest.raises(ValueError, match="partition"):
        be.row_neighbors(W[:5], 2, 2, X[:3])                          # another M
    for k, p in ((0, 1), (33, 1), (1, 0), (1, 7)):
        with pytest.raises(ValueError, match="need 1 <="):
            be.row_neighbors(W, k, p, X[:3])
    be.load(X)
    with pytest.raises(ValueError, match="partition"):
        be.row_neighbors(W, 2, 2, X[:3])


# ---- the C entries: argument errors are status codes, without a GPU ---------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _native.load()


def _scan(lib, d=8, ldx=8, ldq=8, M=5, n_probe=2, k=3, xt=0, qt=1, N=10, Nq=2):
    return lib.dbgsom_ctx_scan_cells_device(None, None, xt, N, d, ldx, None, None, M, None, qt, Nq, ldq, None, n_probe, k,
                                            None, None)


def _query(lib, device, d=8, M=5, n_probe=2, k=3, qt=0, Nq=2, ldq=8):
    if device:
        return lib.dbgsom_ctx_row_neighbors_query_device(None, None, qt, Nq, d, ldq, None, M, n_probe, k, None, None)
    return lib.dbgsom_ctx_row_neighbors_query(None, None, qt, Nq, d, None, M, n_probe, k, None, None)


def test_entry_argument_errors_are_status_codes(lib):
    EINVAL = -1
    for name in ("dbgsom_ctx_scan_cells_device", "dbgsom_ctx_row_neighbors_query", "dbgsom_ctx_row_neighbors_query_device",
                 "dbgsom_ctx_read_partition"):
        assert name in _native.SIGNATURES
    assert _native.MAX_SCAN_FEATURES == rn.MAX_SCAN_FEATURES == 8192
    cases = [(dict(d=8193, ldx=8193, ldq=8193), b"8192"), (dict(d=0), b"shape"), (dict(ldx=7), b"ldx"), (dict(ldq=7), b"ldq"),
             (dict(k=0), b"k <="), (dict(k=33), b"k <="), (dict(n_probe=0), b"n_probe"), (dict(n_probe=6), b"n_probe"),
             (dict(M=40, n_probe=33), b"n_probe"), (dict(M=0), b"M"), (dict(xt=2), b"dtype"), (dict(qt=7), b"dtype"),
             (dict(N=-1), b"shape")]
    for kw, word in cases:
        assert _scan(lib, **kw) == EINVAL and word in lib.dbgsom_last_error(), kw
    assert _scan(lib) == EINVAL and b"null context" in lib.dbgsom_last_error()
    for device in (False, True):
        for kw, word in [(dict(d=8193, ldq=8193), b"8192"), (dict(k=33), b"k <="), (dict(n_probe=6), b"n_probe"),
                         (dict(qt=2), b"dtype"), (dict(M=0), b"M")]:
            assert _query(lib, device, **kw) == EINVAL and word in lib.dbgsom_last_error(), kw
        assert _query(lib, device) == EINVAL and b"null context" in lib.dbgsom_last_error()
    assert _query(lib, True, ldq=7) == EINVAL and b"ldq" in lib.dbgsom_last_error()
    assert lib.dbgsom_ctx_read_partition(None, None, None) == EINVAL and b"null context" in lib.dbgsom_last_error()
