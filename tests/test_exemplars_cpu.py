"""CPU: prototype_exemplars -- the oracle of the selection down the columns against a plain Python sort and as a fold,
the estimator plumbing on a CPU stand-in backend with the invariants of the interface, every refusal by its message,
and the argument errors of the new ABI calls as status codes."""
import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd.backend import HotPathBackend
from tests import exemplars as ex
from tests import golden_inputs as gi
from tests import kneighbors as kn
from tests.test_missing_cpu import punch

ORACLE_CASES = [c for c in ex.COLS_CASES if c[0] <= 300][::3]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the oracle -----------------------------------------------------------------------------------------------------
def _python_sort(R, k, owner, row0):
    """the k smallest (r, i) tuples per column by Python's own sort"""
    N, M = R.shape
    out_r, out_i = np.full((M, k), np.inf), np.full((M, k), -1, dtype=np.int64)
    for j in range(M):
        pairs = sorted((float(R[i, j]), row0 + i) for i in range(N)
                       if R[i, j] < np.inf and (owner is None or owner[i] == j))[:k]
        for t, (r, i) in enumerate(pairs):
            out_r[j, t], out_i[j, t] = r, i
    return out_r, out_i


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[ex.COLS_IDS[ex.COLS_CASES.index(c)] for c in ORACLE_CASES])
def test_oracle_is_a_plain_sort_of_tuples(case):
    N, M, k, kind = case
    R, owner = ex.cols_matrix(case), ex.cols_owner(case)
    got = ex.topk_cols_oracle(R, k, owner, row0=17)
    want = _python_sort(R, k, owner, 17)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    filled = got[1] >= 0
    assert (got[0][filled] < np.inf).all() and np.isposinf(got[0][~filled]).all()
    assert (got[0][:, 1:][filled[:, 1:]] >= got[0][:, :-1][filled[:, 1:]]).all()      # ascending, filled from the left
    assert not (filled[:, 1:] & ~filled[:, :-1]).any()


def test_oracle_on_special_columns():
    inf, nan = np.inf, np.nan
    R = np.array([[2.0, nan, 1.0, inf],
                  [1.0, inf, 1.0, 3.0],
                  [1.0, nan, 1.0, nan],
                  [4.0, inf, 0.5, 2.0]])
    r, i = ex.topk_cols_oracle(R, 3)
    assert np.array_equal(i, [[1, 2, 0], [-1, -1, -1], [3, 0, 1], [3, 1, -1]])     # equal r: the lower row
    assert np.array_equal(r, [[1.0, 1.0, 2.0], [inf] * 3, [0.5, 1.0, 1.0], [2.0, 3.0, inf]])
    assert np.array_equal(ex.owners_of(R), [2, 0, 0, 2])
    r, i = ex.topk_cols_oracle(R, 2, owner=ex.owners_of(R))
    assert np.array_equal(i, [[1, 2], [-1, -1], [3, 0], [-1, -1]])
    assert np.array_equal(ex.owners_of(np.array([[nan, inf], [inf, 7.0]])), [-1, 1])
    # two different r under one square root: the smaller first, whatever the rows
    R = np.array([[1.0 + 2.0 ** -52], [1.0]])
    dist, idx = ex.exemplars_oracle(R, 2)
    assert np.array_equal(idx, [[1, 0]]) and np.array_equal(dist, [[1.0, 1.0]])


@pytest.mark.parametrize("case", ORACLE_CASES[::2], ids=[ex.COLS_IDS[ex.COLS_CASES.index(c)] for c in ORACLE_CASES[::2]])
def test_oracle_folds(case):
    N, M, k, kind = case
    R, owner = ex.cols_matrix(case), ex.cols_owner(case)
    whole = ex.topk_cols_oracle(R, k, owner, row0=5)
    cuts = [0, N // 7, N // 7 + (N + 1) // 2, N]                    # three blocks of uneven size (some may be empty)
    state = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        state = ex.topk_cols_oracle(R[a:b], k, None if owner is None else owner[a:b], row0=5 + a, state=state)
    assert np.array_equal(_bits(state[0]), _bits(whole[0])) and np.array_equal(state[1], whole[1])


def test_tables_reach_what_they_claim():
    cases = ex.COLS_CASES
    long = set(ex.COLS_LONG)
    assert {c[1] for c in cases if c not in long} == set(ex.COLS_M)
    assert {c[0] for c in cases if c not in long} == set(ex.COLS_N)
    assert all(ex.merge_parts(c[0], c[2]) == 1 for c in cases if c not in long)
    assert [ex.merge_parts(c[0], c[2]) for c in ex.COLS_LONG] == [1, 5, 5, 5, 5, 5]
    assert {kn.k_instance(c[2]) for c in ex.COLS_LONG if ex.merge_parts(c[0], c[2]) > 1} == {1, 4, 8, 16, 32}
    assert {(c[1], c[2]) for c in cases} >= {(M, k) for M in ex.COLS_M for k in ex.COLS_K}
    assert {(kn.k_instance(c[2]), c[3]) for c in cases} == {(K, o) for K in kn.K_INSTANCES for o in ex.OWNER_KINDS}
    for K in (8, 16, 32):                                               # every N, so both ends of every segment length
        assert {c[0] for c in cases if kn.k_instance(c[2]) == K} >= set(ex.COLS_N)
        s = ex.segment_rows(K)
        assert {s - 1, s, s + 1} <= set(ex.COLS_N)
    assert [ex.segment_rows(k) for k in (1, 8, 9, 16, 17, 32)] == [64, 64, 128, 128, 256, 256]
    assert any(c[0] < c[2] for c in cases) and len(cases) < 100
    assert sum(c[0] * c[1] for c in cases) < 6e6                       # the whole table is a few tens of megabytes
    assert ex.SLAB_CASE[1] == 300


# ---- estimator plumbing on the stand-in -----------------------------------------------------------------------------
FIT_KW = dict(random_state=0, n_iter=15, max_neurons=20)


@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=ex.ExemplarsOracleBackend(), **FIT_KW).fit(X)
    return est, X


def _check_invariants(est, X, k, dist, idx, own_cell):
    """the invariants of the interface, on dense host rows X"""
    M = len(est.weights_)
    assert dist.shape == idx.shape == (M, k) and dist.dtype == np.float64 and idx.dtype == np.int64
    D = est.prototype_distances(X)
    filled = idx >= 0
    jj = np.broadcast_to(np.arange(M)[:, None], idx.shape)
    assert np.array_equal(_bits(dist[filled]), _bits(D[idx[filled], jj[filled]]))
    assert np.isposinf(dist[~filled]).all() and (idx[~filled] == -1).all()
    assert (dist[:, 1:][filled[:, 1:]] >= dist[:, :-1][filled[:, 1:]]).all()
    units = est.kneighbors(X, 1, return_distance=False)[:, 0]
    if own_cell:
        assert np.array_equal(units[idx[filled]], jj[filled])
        assert np.array_equal(filled.sum(axis=1), np.minimum(k, np.bincount(units, minlength=M)))
        for j in np.flatnonzero(filled[:, 0]):
            assert dist[j, 0] == D[units == j, j].min()
    else:
        assert np.array_equal(filled.sum(axis=1), np.full(M, min(k, len(X))))
        assert np.array_equal(dist[:, 0], D.min(axis=0))


def test_host_array_csr_shapes_and_invariants(fitted):
    est, X = fitted
    be = est._engine()
    be.exemplar_calls = []
    Xq = X[:150]
    for k, own in ((1, False), (4, False), (3, True), (32, True)):
        dist, idx = est.prototype_exemplars(Xq, n_exemplars=k, own_cell=own)
        assert isinstance(dist, np.ndarray) and isinstance(idx, np.ndarray)
        _check_invariants(est, Xq, k, dist, idx, own)
        only = est.prototype_exemplars(Xq, n_exemplars=k, own_cell=own, return_distance=False)
        assert np.array_equal(only, idx)
    assert be.exemplar_calls[::2] == [(150, 1, False), (150, 4, False), (150, 3, True), (150, 32, True)]
    assert np.array_equal(est.prototype_exemplars(Xq)[1], est.prototype_exemplars(Xq, 1, False)[1])   # the defaults
    assert est.prototype_exemplars(Xq, np.int64(2))[0].shape == (len(est.weights_), 2)
    Xs = np.where(np.abs(Xq) < 2.0, 0.0, Xq).astype(np.float32)
    dist, idx = est.prototype_exemplars(Xs, 5, own_cell=True)
    for fmt in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        got = est.prototype_exemplars(fmt(Xs), 5, own_cell=True)
        assert np.array_equal(_bits(got[0]), _bits(dist)) and np.array_equal(got[1], idx)
    Xi = np.rint(Xq[:20]).astype(np.int64)                  # anything but float32 becomes float64, as for predict
    assert np.array_equal(est.prototype_exemplars(Xi, 2)[1], est.prototype_exemplars(Xi.astype(np.float64), 2)[1])


def test_more_exemplars_than_rows_and_no_rows(fitted):
    est, X = fitted
    M = len(est.weights_)
    be = est._engine()
    dist, idx = est.prototype_exemplars(X[:3], n_exemplars=8)
    _check_invariants(est, X[:3], 8, dist, idx, False)
    assert (np.sort(idx[:, :3], axis=1) == np.arange(3)).all() and (idx[:, 3:] == -1).all()
    be.exemplar_calls = []
    for empty in (X[:0], np.empty((0, X.shape[1]))):
        for own in (False, True):
            dist, idx = est.prototype_exemplars(empty, 4, own_cell=own)
            assert dist.shape == idx.shape == (M, 4) and dist.dtype == np.float64 and idx.dtype == np.int64
            assert np.isposinf(dist).all() and (idx == -1).all()
    assert be.exemplar_calls == []                         # no launch


def test_classifier_inherits_it():
    X, y = gi.blobs_f32(300, 5, 4, n_centers=3)
    clf = SomClassifier(backend=ex.ExemplarsOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    dist, idx = clf.prototype_exemplars(X[:80], 3, own_cell=True)
    _check_invariants(clf, X[:80], 3, dist, idx, True)


def test_refusals_and_their_messages(fitted):
    est, X = fitted
    with pytest.raises(NotFittedError):
        SomVQ(backend=ex.ExemplarsOracleBackend()).prototype_exemplars(X)
    call = est.prototype_exemplars
    with pytest.raises(ValueError, match="X has 5 features, but SomVQ is expecting 8 features as input"):
        call(X[:10, :5])
    with pytest.raises(ValueError, match="features"):
        call(sp.csr_matrix(X[:10, :5]))
    with pytest.raises(ValueError, match="features"):
        call(np.empty((0, 3)))
    for bad in (True, np.True_, 2.0, "2", None, [1]):
        with pytest.raises(ValueError, match="n_exemplars does not take .* value, enter integer value"):
            call(X[:10], n_exemplars=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="Expected n_exemplars > 0. Got %d" % bad):
            call(X[:10], n_exemplars=bad)
    with pytest.raises(ValueError, match="n_exemplars = 33 is above the 32 .*prototype_distances"):
        call(X[:10], n_exemplars=33)
    assert call(X[:10], n_exemplars=32)[0].shape[1] == 32
    with pytest.raises(ValueError, match="NaN"):
        call(punch(X[:40], 0.3, 3))
    for missing in ("nan", "nan-fit"):
        holes = SomVQ(backend=ex.ExemplarsOracleBackend(), missing_values=missing, **FIT_KW).fit(X)
        assert holes.prototype_exemplars(X[:10], 2)[0].shape[1] == 2
        with pytest.raises(ValueError, match="impute them first"):
            holes.prototype_exemplars(punch(X[:40], 0.3, 3))
    for metric, label in (("manhattan", "Manhattan"), ("cosine", "cosine")):
        other = SomVQ(backend=ex.ExemplarsOracleBackend(), **FIT_KW)
        other.__dict__.update(est.__dict__)
        other.metric = metric
        with pytest.raises(ValueError, match=r"metric='%s' \(%s\) does not support prototype_exemplars.*squared Euclidean"
                                             % (metric, label)):
            other.prototype_exemplars(X[:10])


def test_base_backend_has_no_exemplars():
    with pytest.raises(NotImplementedError):
        HotPathBackend().exemplars(np.zeros((2, 3)), 1, np.zeros((4, 3)))


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()   # noqa: E731
    one = 16                                # any non-null aligned address: argument errors come before any device work

    assert lib.dbgsom_topk_cols_workspace_bytes(0, 5, 1) == 0 and lib.dbgsom_topk_cols_workspace_bytes(10, 5, 33) == 0
    for k in (1, 8, 9, 32):
        K, S = kn.k_instance(k), -(-1000 // ex.segment_rows(k))
        assert lib.dbgsom_topk_cols_workspace_bytes(1000, 70, k) == (70 * S * K * 8 + 255) // 256 * 256 + (70 * S * K * 4 + 255) // 256 * 256
    for N, M, k, _ in ex.COLS_CASES[::5] + ex.COLS_LONG + [(100000, 25, 8, ""), (65536, 100, 32, ""), (8192, 1024, 32, "")]:
        assert lib.dbgsom_topk_cols_workspace_bytes(N, M, k) == ex.fold_scratch_bytes(N, M, k)
    need = lib.dbgsom_topk_cols_workspace_bytes(10, 5, 2)
    fold = lambda N=10, M=5, ldr=5, own=None, row0=0, k=2, p=one, st=one, w=one, ws=need: (   # noqa: E731
        lib.dbgsom_topk_cols(p, N, M, ldr, own, row0, k, st, st, w, ws, None))
    assert fold(M=0, ldr=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert fold(M=_native.MAX_PROTOTYPES + 1, ldr=20000) == -1 and b"MAX_PROTOTYPES" in err()
    assert fold(k=0) == -1 and b"k >= 1" in err()
    assert fold(k=33) == -1 and b"MAX_NEIGHBORS" in err()
    assert fold(ldr=4) == -1 and b"ldr" in err()
    assert fold(N=-1) == -1 and b"shape" in err()
    assert fold(row0=-1) == -1 and b"row0" in err()
    assert fold(row0=2 ** 31 - 10) == -1 and b"row0 + N" in err()
    assert fold(row0=2 ** 31 - 11, ws=need - 1) == -3        # row0 + N = 2^31 - 1 passes: the short workspace is met
    assert fold(p=None) == -1 and b"null pointer" in err()
    assert fold(st=None) == -1 and b"null pointer" in err()
    assert fold(w=None) == -1 and b"null pointer" in err()
    assert fold(p=20) == -1 and b"aligned" in err()
    assert fold(own=20) == -1 and b"aligned" in err()
    assert fold(st=20) == -1 and b"aligned" in err()
    assert fold(w=24) == -1 and b"16-byte aligned" in err()
    assert fold(ws=need - 1) == -3 and (b"%d bytes, %d needed" % (need - 1, need)) in err()
    assert fold(N=0, p=None, st=None, w=None, ws=0) == 0     # no rows: the state stays what it is
    assert fold(k=6, M=5) == -3                              # k may exceed M (and N): only the workspace is short

    init = lambda M=5, k=2, st=one: lib.dbgsom_topk_cols_init(st, st, M, k, None)   # noqa: E731
    assert init(M=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert init(k=0) == -1 and init(k=33) == -1 and b"MAX_NEIGHBORS" in err()
    assert init(st=None) == -1 and b"null pointer" in err()
    assert init(st=20) == -1 and b"aligned" in err()

    need = lib.dbgsom_exemplars_workspace_bytes(10, 5, 2, 0)
    assert need == (lib.dbgsom_kneighbors_workspace_bytes(10, 5, 0) + 2 * 256 + lib.dbgsom_topk_cols_workspace_bytes(10, 5, 2)
                    + 2 * 256)                              # the slab, the units of a slab (twice), the scratch, the state
    full = lambda dt=0, N=10, d=4, ldx=4, M=5, k=2, slab=0, p=one, o=one, w=one, ws=need: (   # noqa: E731
        lib.dbgsom_exemplars(p, dt, N, d, ldx, p, p, M, p, k, 1, slab, o, o, w, ws, None))
    assert full(dt=7) == -1 and b"x_dtype" in err()
    assert full(ldx=3) == -1 and b"shape" in err()
    assert full(M=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert full(k=0) == -1 and b"k >= 1" in err()
    assert full(k=33) == -1 and b"MAX_NEIGHBORS" in err()
    assert full(slab=-1) == -1 and b"slab_rows" in err()
    assert full(p=None) == -1 and b"null pointer" in err()
    assert full(o=None) == -1 and b"null pointer" in err()
    assert full(w=None) == -1 and b"null pointer" in err()
    assert full(o=20) == -1 and b"aligned" in err()
    assert full(w=24) == -1 and b"16-byte aligned" in err()
    assert full(ws=need - 1) == -3 and (b"%d bytes, %d needed" % (need - 1, need)) in err()

    W = np.zeros((5, 4))
    out = np.zeros(64)
    w = W.ctypes.data
    calls = (("dbgsom_ctx_exemplars_query", lambda c, M, k: (c, one, 0, 10, 4, w, M, k, 0, one, one)),
             ("dbgsom_ctx_exemplars_query_device", lambda c, M, k: (c, one, 0, 10, 4, 4, w, M, k, 0, one, one)),
             ("dbgsom_ctx_exemplars_query_csr", lambda c, M, k: (c, one, one, one, 0, 10, 4, 3, w, M, k, 1, one, one)))
    for name, args in calls:
        assert getattr(lib, name)(*args(None, 5, 2)) == -1 and b"null context" in err()
        with pytest.raises(ValueError, match="null context"):
            _native.call(name, *args(None, 5, 2))
        assert getattr(lib, name)(*args(out.ctypes.data, 0, 2)) == -1 and b"MAX_PROTOTYPES" in err()   # (before the context is touched)
        assert getattr(lib, name)(*args(out.ctypes.data, 5, 0)) == -1 and b"k >= 1" in err()
        assert getattr(lib, name)(*args(out.ctypes.data, 5, 33)) == -1 and b"MAX_NEIGHBORS" in err()
    assert lib.dbgsom_ctx_exemplars_query_device(out.ctypes.data, one, 0, 10, 4, 3, w, 5, 2, 0, one, one) == -1 and b"ldx" in err()
