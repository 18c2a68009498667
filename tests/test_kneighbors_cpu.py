"""CPU: kneighbors -- the oracle's order against the search's own oracle, the shape tables against the launcher paths
they claim to cover, the workspace size, the estimator plumbing on a CPU stand-in backend, and the argument errors of
the new ABI calls as status codes."""
import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd.backend import HotPathBackend
from oracle import som_oracle as o
from tests import device_abi as da
from tests import golden_inputs as gi
from tests import kneighbors as kn
from tests import prototype_distances as pd
from tests.test_missing_cpu import GAP, case as masked_case, masked_distances, punch


# ---- the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pd.CASES, ids=pd.CASE_IDS)
def test_oracle_order_is_the_search_oracles(case):
    X, W, D = pd.case_data(case)
    Xw = da.widen(X)
    _, i1 = o.bmu_chain(Xw, W, 1)
    assert np.array_equal(kn.topk_oracle(X, W, 1, D)[:, 0], i1)
    if W.shape[0] >= 2:
        _, i2 = o.bmu_chain(Xw, W, 2)
        assert np.array_equal(kn.topk_oracle(X, W, 2, D), i2)
    k = min(W.shape[0], 32)
    idx = kn.topk_oracle(X, W, k, D)
    got = np.take_along_axis(D, idx, axis=1)
    assert (np.diff(got, axis=1) >= 0).all() and np.array_equal(got, np.sort(D, axis=1)[:, :k])
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all()     # no prototype twice


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_planted_collapse(dt):
    """two different r under one square root: the smaller r first, although its index is the higher"""
    X = kn.COLLAPSE_X.astype(dt)
    d2, i2 = o.bmu_chain(X, kn.COLLAPSE_W, 2)
    assert np.array_equal(d2, [[1.0, 1.0]]) and np.array_equal(i2, [[1, 0]])
    D = pd.pair_distances(X, kn.COLLAPSE_W)
    assert np.array_equal(D, [[1.0, 1.0, 3.0]])
    assert np.array_equal(np.argsort(D, axis=1, kind="stable"), [[0, 1, 2]])       # what a sort of D alone would say
    assert np.array_equal(kn.topk_oracle(X, kn.COLLAPSE_W, 3), [[1, 0, 2]])
    assert np.array_equal(kn.topk_oracle(X, kn.COLLAPSE_W, 2), [[1, 0]])
    assert np.array_equal(kn.topk_oracle(X, kn.COLLAPSE_W, 1), [[1]])


def test_lexsort_reference_on_a_small_matrix():
    R = np.array([[4.0, 1.0, np.nan, 1.0, np.inf, 0.25], [np.inf, np.nan, 9.0, np.inf, np.nan, np.inf]])
    dist, idx = kn.topk_lexsort(R, 4)
    assert np.array_equal(idx, [[5, 1, 3, 0], [2, -1, -1, -1]])
    assert np.array_equal(dist, [[0.5, 1.0, 1.0, 2.0], [3.0, np.inf, np.inf, np.inf]])


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("frac", pd.MASKED_FRACS)
@pytest.mark.parametrize("N,d,M", pd.MASKED_SHAPES)
def test_masked_inputs_have_no_near_ties_among_the_reported(N, d, M, frac, dt):
    """the masked oracle is NumPy's direct form and the device agrees with it within RTOL = 1e-12, not bit for bit:
    indices can be compared only where neighbouring distances of the order are further apart than that"""
    X, W, D = masked_case(N, d, M, frac, dt)
    k = min(M, 32)
    head = np.sort(D, axis=1)[:, :min(k + 1, M)]
    if head.shape[1] > 1:
        assert (np.diff(head, axis=1) > GAP * head[:, 1:]).all()


# ---- the tables -------------------------------------------------------------------------------------------------------
def test_tables_reach_every_instantiation_and_path():
    pairs = lambda a, b: {(c[a], c[b]) for c in kn.TOPK_CASES}   # noqa: E731
    assert pairs(1, 2) == {(M, k) for M in kn.TOPK_M for k in kn.TOPK_K if k <= M}
    assert pairs(0, 1) == {(N, M) for N in kn.TOPK_N for M in kn.TOPK_M if M > 1} | {(1, 1)}
    assert pairs(0, 2) == {(N, k) for N in kn.TOPK_N for k in kn.TOPK_K}
    assert {c[3] for c in kn.TOPK_CASES} == {0, 3}
    assert {(c[3], c[1]) for c in kn.TOPK_CASES if c[1] > 1} == {(p, M) for p in (0, 3) for M in kn.TOPK_M if M > 1}
    assert {kn.k_instance(c[2]) for c in kn.TOPK_CASES} == set(kn.K_INSTANCES)
    # more than one pass of the four-load loop (M > 256), lanes without an entry (M < 64), a second workgroup (N > 4)
    assert any(c[1] > 256 for c in kn.TOPK_CASES) and any(c[1] < 64 for c in kn.TOPK_CASES)
    # dbgsom_kneighbors: every k on both launcher forms and both stores of the slab; every instantiation but K = 4,
    # which k = 3 and 4 of the table above reach
    reached = {(pd.launcher_form(c)[0][0], k) for i, c in enumerate(pd.CASES) for k in kn.case_ks(i)}
    stores = {(w, k) for i, c in enumerate(pd.CASES) for k in kn.case_ks(i) for w in kn.slab_stores(c)}
    for k in kn.KN_K:
        assert {("dma", k), ("reg", k)} <= reached and {("16", k), ("8", k)} <= stores
    assert {kn.k_instance(k) for i in range(len(pd.CASES)) for k in kn.case_ks(i)} == {1, 2, 8, 16, 32}
    assert all(1 <= k <= min(c[2], kn.MAX_NEIGHBORS) for i, c in enumerate(pd.CASES) for k in kn.case_ks(i))
    assert any(c[2] % 2 for c in pd.CASES)                       # an odd M: the slab's rows are padded to even
    # a slab boundary inside the rows, the last slab short
    assert kn.SLAB_CASE in pd.CASES and kn.SLAB_CASE[1] == 300 and 300 % 128


def test_limits_agree_with_the_header():
    assert kn.MAX_NEIGHBORS == _native.MAX_NEIGHBORS == max(kn.K_INSTANCES)
    assert "#define DBGSOM_MAX_NEIGHBORS %d\n" % _native.MAX_NEIGHBORS in open(_native.HEADER).read()


def test_workspace_does_not_grow_with_the_rows():
    lib = _native.load()
    big = lib.dbgsom_kneighbors_workspace_bytes(10**6, 1024, 0)
    assert big == lib.dbgsom_kneighbors_workspace_bytes(10**5, 1024, 0)
    assert 0 < big <= (64 << 20) + 1024 * 8
    assert lib.dbgsom_kneighbors_workspace_bytes(10**6, 1023, 0) <= (64 << 20) + 1024 * 8
    assert lib.dbgsom_kneighbors_workspace_bytes(10**6, 1, 0) <= (64 << 20) + 2 * 8
    assert lib.dbgsom_kneighbors_workspace_bytes(10**6, 100, 0) == 65536 * 100 * 8   # whole grids of the product kernel
    assert lib.dbgsom_kneighbors_workspace_bytes(300, 101, 128) == 128 * 102 * 8      # M rounded up to even
    assert lib.dbgsom_kneighbors_workspace_bytes(100, 101, 128) <= 100 * 102 * 8 + 256   # never more than the rows
    assert lib.dbgsom_kneighbors_workspace_bytes(0, 101, 0) == 0
    # the largest map: 524 rows would fit, 512 are taken
    assert lib.dbgsom_kneighbors_workspace_bytes(10**6, 16000, 0) == 512 * 16000 * 8
    m = lib.dbgsom_kneighbors_masked_workspace_bytes(0, 10**6, 64, 129, 0)
    assert m == lib.dbgsom_kneighbors_masked_workspace_bytes(0, 10**5, 64, 129, 0)


# ---- estimator plumbing on the stand-in ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=kn.KNeighborsOracleBackend(), missing_values="nan", random_state=0, n_iter=15,
                max_neurons=20).fit(X)
    return est, X


def test_shapes_dtypes_and_what_follows_from_the_order(fitted):
    est, X = fitted
    M = len(est.weights_)
    dist, idx = est.kneighbors(X[:90])
    assert dist.shape == idx.shape == (90, 5) and dist.dtype == np.float64 and idx.dtype == np.int64
    D = est.prototype_distances(X[:90])
    assert np.array_equal(dist, np.take_along_axis(D, idx, axis=1)) and (np.diff(dist, axis=1) >= 0).all()
    assert np.array_equal(idx[:, 0], est.predict(X[:90]))
    d2, i2 = est._get_winning_neurons(X[:90], 2)
    assert np.array_equal(idx[:, :2], i2) and np.array_equal(dist[:, :2], d2)
    only = est.kneighbors(X[:90], return_distance=False)
    assert isinstance(only, np.ndarray) and np.array_equal(only, idx)
    dM, iM = est.kneighbors(X[:90], n_neighbors=M)
    assert np.array_equal(np.sort(iM, axis=1), np.tile(np.arange(M), (90, 1))) and np.array_equal(dM, np.sort(D, axis=1))
    assert np.array_equal(est.kneighbors(X[:90], np.int64(3))[1], idx[:, :3])
    Xi = np.rint(X[:20]).astype(np.int64)                 # anything but float32 becomes float64, as for predict
    assert np.array_equal(est.kneighbors(Xi, 4)[1], kn.topk_oracle(Xi.astype(np.float64), est.weights_, 4))


def test_classifier_inherits_it():
    X, y = gi.blobs_f32(300, 5, 4, n_centers=3)
    clf = SomClassifier(backend=kn.KNeighborsOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    dist, idx = clf.kneighbors(X[:30], 3)
    assert np.array_equal(idx, kn.topk_oracle(X[:30], clf.weights_, 3))
    assert np.array_equal(dist, np.take_along_axis(pd.pair_distances(X[:30], clf.weights_), idx, axis=1))


def test_refusals_and_their_messages(fitted):
    est, X = fitted
    M = len(est.weights_)
    with pytest.raises(NotFittedError):
        SomVQ(backend=kn.KNeighborsOracleBackend()).kneighbors(X)
    with pytest.raises(ValueError, match="features"):
        est.kneighbors(X[:10, :5])
    with pytest.raises(ValueError, match="features"):
        est.kneighbors(sp.csr_matrix(X[:10, :5]))
    with pytest.raises(ValueError, match="features"):
        est.kneighbors(np.empty((0, 3)))
    for bad in (2.0, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="n_neighbors does not take .* value, enter integer value"):
            est.kneighbors(X[:10], bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match=r"Expected n_neighbors > 0. Got %d" % bad):
            est.kneighbors(X[:10], bad)
    with pytest.raises(ValueError, match=r"Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, "
                                         r"n_samples_fit = %d .*n_samples = 10" % (M + 1, M)):
        est.kneighbors(X[:10], M + 1)
    be = est._engine()
    be.kneighbors_rows = []
    wide = SomVQ(backend=be, random_state=0)              # a map of 40 prototypes: 33 is within it, above the limit
    wide.weights_ = np.random.default_rng(0).normal(size=(40, X.shape[1]))
    wide.n_features_in_ = X.shape[1]
    with pytest.raises(ValueError, match="prototype_distances"):
        wide.kneighbors(X[:10], 33)
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit"):
        wide.kneighbors(X[:10], 41)
    assert wide.kneighbors(X[:10], 32)[1].shape == (10, 32) and be.kneighbors_rows == [10]
    plain = SomVQ(backend=kn.KNeighborsOracleBackend(), random_state=0, n_iter=15, max_neurons=20).fit(X)
    Xn = punch(X[:40], 0.3, 3)
    with pytest.raises(ValueError, match="NaN"):
        plain.kneighbors(Xn)
    with pytest.raises(ValueError, match="no observed entry"):
        est.kneighbors(np.vstack([Xn, np.full((1, X.shape[1]), np.nan, dtype=X.dtype)]))
    with pytest.raises(ValueError, match="[Ii]nf"):
        est.kneighbors(np.where(np.isnan(Xn), np.inf, Xn))


def test_split_and_scatter(fitted):
    est, X = fitted
    be = est._engine()
    Xn = punch(X[:200], 0.3, 2)
    Xn[::3] = X[:200:3]                                   # every third row complete
    incomplete = np.isnan(Xn).any(axis=1)
    be.kneighbors_rows, be.masked_kneighbors_rows = [], []
    dist, idx = est.kneighbors(Xn, 4)
    assert be.masked_kneighbors_rows == [int(incomplete.sum())] and be.kneighbors_rows == [int((~incomplete).sum())]
    md, mi = kn.masked_topk(Xn[incomplete], est.weights_, 4)
    assert np.array_equal(idx[incomplete], mi) and np.array_equal(dist[incomplete], md)
    assert np.array_equal(idx[~incomplete], kn.topk_oracle(Xn[~incomplete], est.weights_, 4))
    assert np.array_equal(dist, np.take_along_axis(est.prototype_distances(Xn), idx, axis=1))
    assert np.array_equal(md, np.sort(masked_distances(Xn[incomplete], est.weights_), axis=1)[:, :4])
    assert np.array_equal(idx[:, 0], est.predict(Xn))
    # no incomplete row: no masked call; nothing but incomplete rows: no dense call
    be.kneighbors_rows, be.masked_kneighbors_rows = [], []
    est.kneighbors(X[:50])
    assert be.masked_kneighbors_rows == [] and be.kneighbors_rows == [50]
    be.kneighbors_rows, be.masked_kneighbors_rows = [], []
    only = est.kneighbors(Xn[incomplete], 2, return_distance=False)
    assert be.masked_kneighbors_rows == [int(incomplete.sum())] and be.kneighbors_rows == []
    assert np.array_equal(only, mi[:, :2])


def test_sparse_equals_dense(fitted):
    est, X = fitted
    Xs = np.where(np.abs(X[:120]) < 2.0, 0.0, X[:120]).astype(np.float32)
    dist, idx = est.kneighbors(Xs, 3)
    for fmt in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        got = est.kneighbors(fmt(Xs), 3)
        assert np.array_equal(got[0], dist) and np.array_equal(got[1], idx)


def test_empty_input(fitted):
    est, X = fitted
    be = est._engine()
    be.kneighbors_rows, be.masked_kneighbors_rows = [], []
    for empty in (X[:0], np.empty((0, X.shape[1]))):
        dist, idx = est.kneighbors(empty, 3)
        assert dist.shape == idx.shape == (0, 3) and dist.dtype == np.float64 and idx.dtype == np.int64
        only = est.kneighbors(empty, 3, return_distance=False)
        assert only.shape == (0, 3) and only.dtype == np.int64
    assert be.kneighbors_rows == [] and be.masked_kneighbors_rows == []


def test_base_backend_has_no_kneighbors():
    with pytest.raises(NotImplementedError):
        HotPathBackend().kneighbors(np.zeros((2, 3)), 1, np.zeros((4, 3)))
    with pytest.raises(NotImplementedError):
        HotPathBackend().kneighbors_masked(np.zeros((2, 3)), 1, np.zeros((4, 3)))


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()   # noqa: E731
    one = 16                                # any non-null aligned address: argument errors come before any device work

    topk = lambda N=10, M=5, ldr=5, k=3, p=one: lib.dbgsom_topk_rows(p, N, M, ldr, k, p, p, None)   # noqa: E731
    assert topk(k=0) == -1 and b"k" in err()
    assert topk(k=6) == -1 and b"k <= M" in err()
    assert topk(M=40, ldr=40, k=33) == -1 and b"MAX_NEIGHBORS" in err()
    assert topk(ldr=4) == -1 and b"ldr" in err()
    assert topk(M=0, ldr=0) == -1 and b"M" in err()
    assert topk(p=None) == -1 and b"null pointer" in err()
    assert topk(N=0, p=None) == 0           # no rows: nothing to do, nothing dereferenced

    need = lib.dbgsom_kneighbors_workspace_bytes(10, 5, 0)
    assert need >= 10 * 6 * 8
    knn = lambda dt=0, N=10, d=4, ldx=4, M=5, k=3, slab=0, p=one, ws=need: lib.dbgsom_kneighbors(   # noqa: E731
        p, dt, N, d, ldx, p, p, M, p, k, slab, p, p, p, ws, None)
    assert knn(dt=7) == -1 and b"x_dtype" in err()
    assert knn(ldx=3) == -1 and b"shape" in err()
    assert knn(k=0) == -1 and b"k" in err()
    assert knn(k=6) == -1 and b"k <= M" in err()
    assert knn(M=40, k=33) == -1 and b"MAX_NEIGHBORS" in err()
    assert knn(M=_native.MAX_PROTOTYPES + 1) == -1 and b"MAX_PROTOTYPES" in err()
    assert knn(slab=-1) == -1 and b"slab_rows" in err()
    assert knn(p=None) == -1 and b"null pointer" in err()
    assert knn(ws=need - 1) == -3 and (b"%d bytes, %d needed" % (need - 1, need)) in err()
    assert knn(N=0, p=None, ws=0) == 0

    mneed = lib.dbgsom_kneighbors_masked_workspace_bytes(0, 10, 4, 5, 0)
    assert mneed >= lib.dbgsom_bmu_masked_workspace_bytes(0, 10, 4, 5) + need
    masked = lambda dt=0, N=10, d=4, ldx=4, M=5, ldw=4, k=3, slab=0, p=one, ws=mneed: lib.dbgsom_kneighbors_masked(   # noqa: E731
        p, dt, N, d, ldx, p, M, ldw, k, slab, p, p, p, ws, None)
    assert masked(dt=2) == -1 and b"x_dtype" in err()          # no bfloat16 rows with holes, as for the search
    assert masked(k=0) == -1 and b"k" in err()
    assert masked(k=6) == -1 and b"k <= M" in err()
    assert masked(M=40, k=33) == -1 and b"MAX_NEIGHBORS" in err()
    assert masked(ldw=3) == -1 and b"ldw" in err()
    assert masked(p=None) == -1 and b"null pointer" in err()
    assert masked(ws=mneed - 1) == -3 and (b"%d bytes, %d needed" % (mneed - 1, mneed)) in err()
    assert masked(N=0, p=None, ws=0) == 0

    W = np.zeros((5, 4))
    out = np.zeros(64)
    calls = (("dbgsom_ctx_kneighbors_query", lambda c, k: (c, one, 0, 10, 4, W.ctypes.data, 5, k, one, one)),
             ("dbgsom_ctx_kneighbors_query_device", lambda c, k: (c, one, 0, 10, 4, 4, W.ctypes.data, 5, k, one, one)),
             ("dbgsom_ctx_kneighbors_query_csr", lambda c, k: (c, one, one, one, 0, 10, 4, 3, W.ctypes.data, 5, k, one, one)),
             ("dbgsom_ctx_kneighbors_query_masked", lambda c, k: (c, one, 0, 10, 4, W.ctypes.data, 5, k, one, one)))
    for name, args in calls:
        assert getattr(lib, name)(*args(None, 3)) == -1 and b"null context" in err()
        with pytest.raises(ValueError, match="null context"):
            _native.call(name, *args(None, 3))
        assert getattr(lib, name)(*args(out.ctypes.data, 0)) == -1 and b"k" in err()    # (before the context is touched)
        assert getattr(lib, name)(*args(out.ctypes.data, 6)) == -1 and b"k <= M" in err()
