"""CPU: the distortion measure -- the restatement of the energy kernel against np.longdouble sums, the exact squared
matrix against the oracle's distances and winners, the estimator plumbing on a CPU stand-in backend, every refusal by
its message, and the argument errors of the new ABI calls as status codes."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd.backend import HotPathBackend
from oracle import som_oracle as o
from tests import device_abi as da
from tests import distortion as ds
from tests import golden_inputs as gi
from tests import prototype_distances as pd
from tests.test_missing_cpu import punch

TABLE_CASES = [pd.CASES[0], pd.CASES[7], pd.CASES[14], pd.CASES[26]]     # f32 dma, f64 dma, f32 strided, bfloat16


# ---- the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not da.have_longdouble(), reason="np.longdouble has no 64-bit significand here")
@pytest.mark.parametrize("M", ds.BOUND_M)
def test_restatement_is_within_its_bound_of_the_longdouble_sum(M):
    rng = np.random.default_rng(M)
    H = ds.gaussian_factors(M, sigma=2.0)
    worst = 0.0
    for scale in ds.BOUND_SCALES:
        R = rng.random((6, M)) * scale
        b, e = ds.energy_rows(R, H)
        assert np.array_equal(b, np.argmin(R, axis=1))
        ref, bound = ds.longdouble_energy(R, H, b), ds.error_bound(M, H, R, b)
        err = np.abs(np.asarray(e, dtype=np.longdouble) - ref)
        assert (err <= bound).all()
        worst = max(worst, float(np.max(err / bound)))
    print("M = %d: largest error / bound = %.3f" % (M, worst))


def test_restatement_on_special_rows():
    inf, nan = np.inf, np.nan
    R = np.array([[4.0, 1.0, nan, 1.0, inf, 0.25],      # an ordinary row: NaN and +inf enter the sum as they are
                  [inf, nan, inf, inf, nan, inf],       # nothing below +inf
                  [2.0, 1.0, 1.0, 3.0, inf, 5.0],       # equal minima: the lowest index; +inf under h > 0
                  [2.0, 1.0, 1.0, 3.0, 7.0, 5.0]])
    b, e = ds.energy_rows(R, np.ones((6, 6)))
    assert np.array_equal(b, [5, -1, 1, 1])
    assert np.isnan(e[0]) and np.isnan(e[1]) and e[2] == inf and e[3] == 19.0
    b, e = ds.energy_rows(R, np.eye(6))                 # h = 0 against +inf: 0 * inf = NaN
    assert np.array_equal(b, [5, -1, 1, 1]) and np.isnan(e[:3]).all() and e[3] == 1.0


@pytest.mark.parametrize("case", ds.ROWS_CASES, ids=ds.ROWS_IDS)
def test_identity_factors_give_the_winning_value(case):
    N, M = case
    R = np.where(np.isfinite(ds.rows_matrix(case)), ds.rows_matrix(case), 3.0)
    b, e = ds.energy_rows(R, np.eye(M))
    assert np.array_equal(b, np.argmin(R, axis=1)) and np.array_equal(e, R[np.arange(N), b])
    ones_b, ones_e = ds.energy_rows(R, np.ones((M, M)))
    assert np.array_equal(ones_b, b)
    np.testing.assert_allclose(ones_e, R.sum(axis=1), rtol=(-(-M // 64) + 8) * ds.U)


def test_tables_reach_what_they_claim():
    assert {c[1] for c in ds.ROWS_CASES} == set(ds.ROWS_M) and {c[0] for c in ds.ROWS_CASES} == set(ds.ROWS_N)
    assert (300, 2099) in ds.ROWS_CASES and any(N % 4 for N, _ in ds.ROWS_CASES)
    assert any(M > 256 for _, M in ds.ROWS_CASES) and any(M < 64 for _, M in ds.ROWS_CASES)
    for case in ds.ROWS_CASES:
        N, M = case
        R = ds.rows_matrix(case)
        b, e = ds.energy_rows(R, ds.rows_factors(case))
        if N >= ds.ROWS_KINDS:
            assert b[0] == 0 and b[1] == (63 if M > 63 else 0) and b[2] == -1 and np.isnan(e[2])
            assert np.isinf(e[3]) or M == 1
    assert ds.SLAB_CASE in pd.CASES and ds.SLAB_CASE[1] == 300


# ---- the exact squared matrix ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE_CASES, ids=[pd.CASE_IDS[pd.CASES.index(c)] for c in TABLE_CASES])
def test_squared_matrix_is_the_oracles(case):
    X, W, D = pd.case_data(case)
    R, H, b, e = ds.case_reference(case)
    assert np.array_equal(np.sqrt(R).view(np.uint64), D.view(np.uint64))
    _, winners = o.bmu_chain(np.ascontiguousarray(da.widen(X)), W, 1)
    assert np.array_equal(b, np.ravel(winners))
    if W.shape[0] >= 3:                                   # the last prototype duplicates the first: the lowest index wins
        assert np.array_equal(R[:, -1], R[:, 0]) and not (b == W.shape[0] - 1).any()


# ---- estimator plumbing on the stand-in -----------------------------------------------------------------------------
FIT_KW = dict(random_state=0, n_iter=15, max_neurons=20)


@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=ds.DistortionOracleBackend(), **FIT_KW).fit(X)
    return est, X


def _hops(est):
    nodes = list(est.neurons_)
    index = {n: i for i, n in enumerate(nodes)}
    A = np.zeros((len(nodes),) * 2)
    for a, b in est.som_.edges:
        A[index[a], index[b]] = A[index[b], index[a]] = 1.0
    return shortest_path(sp.csr_matrix(A), directed=False, unweighted=True)


def test_sample_and_mean_on_the_stand_in(fitted):
    est, X = fitted
    M = len(est.weights_)
    be = est._engine()
    be.energy_rows, be.energy_H = [], []
    e, bmu = est.sample_distortion(X[:90])
    assert e.shape == bmu.shape == (90,) and e.dtype == np.float64 and bmu.dtype == np.int64
    assert np.array_equal(bmu, est.predict(X[:90]))
    hop = _hops(est)
    assert hop.shape == (M, M) and np.array_equal(hop, est._distance_matrix)
    sigma = est._calculate_current_sigma()
    H = np.exp(-(hop ** 2 / (2 * sigma ** 2)))
    assert be.energy_rows == [90] and np.array_equal(be.energy_H[0].view(np.uint64), H.view(np.uint64))
    want_b, want_e = ds.energy_rows(ds.squared_matrix(X[:90], est.weights_), H)
    assert np.array_equal(bmu, want_b) and np.array_equal(e.view(np.uint64), want_e.view(np.uint64))
    D = est.prototype_distances(X[:90])
    np.testing.assert_allclose(e, (H[bmu] * D ** 2).sum(axis=1), rtol=1e-13)
    assert est.calculate_distortion(X[:90]) == float(np.sum(e)) / 90
    assert est.calculate_distortion(X[:90], sigma=sigma) == est.calculate_distortion(X[:90])
    # a smaller bandwidth shrinks every h; sigma -> 0 leaves the winning value
    small, _ = est.sample_distortion(X[:90], sigma=0.5 * sigma)
    assert (small <= e).all() and (small < e).any()
    tiny, _ = est.sample_distortion(X[:90], sigma=1e-3)
    assert np.array_equal(tiny, D[np.arange(90), bmu] ** 2) or np.allclose(tiny, D[np.arange(90), bmu] ** 2, rtol=1e-15)
    assert np.array_equal(est.sample_distortion(X[:90], sigma=np.float32(2.0))[0], est.sample_distortion(X[:90], 2)[0])
    Xi = np.rint(X[:20]).astype(np.int64)                 # anything but float32 becomes float64, as for predict
    assert np.array_equal(est.sample_distortion(Xi)[1], est.predict(Xi))


def test_factors_follow_the_map_after_dead_units_and_a_pickle():
    X, _ = gi.case_X("blobs_dead")
    est = SomVQ(backend=ds.DistortionOracleBackend(), **gi.EST_KWARGS["blobs_dead"]).fit(X)
    M = len(est.weights_)
    assert np.array_equal(_hops(est), est._distance_matrix) and est._distance_matrix.shape == (M, M)
    e, bmu = est.sample_distortion(X[:50])
    clone = pickle.loads(pickle.dumps(est))
    clone.backend = ds.DistortionOracleBackend()
    e2, bmu2 = clone.sample_distortion(X[:50])
    assert np.array_equal(bmu2, bmu) and np.array_equal(e2.view(np.uint64), e.view(np.uint64))
    assert np.array_equal(clone._engine().energy_H[0], est._engine().energy_H[-1])
    assert clone.calculate_distortion(X[:50]) == est.calculate_distortion(X[:50])


def test_disconnected_components_have_factor_zero(fitted):
    est, X = fitted
    hop = est._distance_matrix
    try:
        cut = hop.copy()
        cut[0, 1:] = cut[1:, 0] = np.inf
        est._distance_matrix = cut
        H = est._neighborhood_factors(1.0)
    finally:
        est._distance_matrix = hop
    assert H[0, 0] == 1.0 and (H[0, 1:] == 0.0).all() and (H[1:, 0] == 0.0).all() and (H[1:, 1:] > 0.0).all()


def test_classifier_inherits_it():
    X, y = gi.blobs_f32(300, 5, 4, n_centers=3)
    clf = SomClassifier(backend=ds.DistortionOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    e, bmu = clf.sample_distortion(X[:30])
    H = clf._neighborhood_factors(None)
    want_b, want_e = ds.energy_rows(ds.squared_matrix(X[:30], clf.weights_), H)
    assert np.array_equal(bmu, want_b) and np.array_equal(e.view(np.uint64), want_e.view(np.uint64))
    assert clf.calculate_distortion(X[:30]) == float(np.sum(e)) / 30


def test_sparse_equals_dense(fitted):
    est, X = fitted
    Xs = np.where(np.abs(X[:120]) < 2.0, 0.0, X[:120]).astype(np.float32)
    e, bmu = est.sample_distortion(Xs)
    for fmt in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        got = est.sample_distortion(fmt(Xs))
        assert np.array_equal(got[0].view(np.uint64), e.view(np.uint64)) and np.array_equal(got[1], bmu)
        assert est.calculate_distortion(fmt(Xs)) == est.calculate_distortion(Xs)


def test_empty_input(fitted):
    est, X = fitted
    be = est._engine()
    be.energy_rows = []
    for empty in (X[:0], np.empty((0, X.shape[1]))):
        e, bmu = est.sample_distortion(empty)                  # as kneighbors: empty results, no launch
        assert e.shape == bmu.shape == (0,) and e.dtype == np.float64 and bmu.dtype == np.int64
        with pytest.raises(ValueError, match="0 sample"):      # as calculate_quantization_error: no mean of nothing
            est.calculate_distortion(empty)
        with pytest.raises(ValueError, match="0 sample"):
            est.calculate_quantization_error(empty)
    assert be.energy_rows == []


def test_refusals_and_their_messages(fitted):
    est, X = fitted
    with pytest.raises(NotFittedError):
        SomVQ(backend=ds.DistortionOracleBackend()).sample_distortion(X)
    with pytest.raises(NotFittedError):
        SomVQ(backend=ds.DistortionOracleBackend()).calculate_distortion(X)
    for call in (est.sample_distortion, est.calculate_distortion):
        with pytest.raises(ValueError, match="X has 5 features, but SomVQ is expecting 8 features as input"):
            call(X[:10, :5])
        with pytest.raises(ValueError, match="features"):
            call(sp.csr_matrix(X[:10, :5]))
        with pytest.raises(ValueError, match="features"):
            call(np.empty((0, 3)))
        for bad in (0, 0.0, -1.0, np.inf, np.nan, "2", True, [1.0]):
            with pytest.raises(ValueError, match="sigma must be None or a finite float > 0"):
                call(X[:10], sigma=bad)
        with pytest.raises(ValueError, match="NaN"):
            call(punch(X[:40], 0.3, 3))
        with pytest.raises(ValueError, match="[Ii]nf"):
            call(np.where(np.isnan(punch(X[:40], 0.3, 3)), np.inf, X[:40]))
    for missing in ("nan", "nan-fit"):
        holes = SomVQ(backend=ds.DistortionOracleBackend(), missing_values=missing, **FIT_KW).fit(X)
        assert holes.sample_distortion(X[:10])[0].shape == (10,)
        for call in (holes.sample_distortion, holes.calculate_distortion):
            with pytest.raises(ValueError, match="impute them first"):
                call(punch(X[:40], 0.3, 3))
    for metric, label in (("manhattan", "Manhattan"), ("cosine", "cosine")):
        other = SomVQ(backend=ds.DistortionOracleBackend(), **FIT_KW)
        other.__dict__.update(est.__dict__)
        other.metric = metric
        for call in (other.sample_distortion, other.calculate_distortion):
            with pytest.raises(ValueError, match=r"metric='%s' \(%s\) does not support .*distortion.*squared Euclidean"
                                                 % (metric, label)):
                call(X[:10])


def test_base_backend_has_no_neighborhood_energy():
    with pytest.raises(NotImplementedError):
        HotPathBackend().neighborhood_energy(np.zeros((2, 3)), np.eye(2), np.zeros((4, 3)))


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()   # noqa: E731
    one = 16                                # any non-null aligned address: argument errors come before any device work

    rows = lambda N=10, M=5, ldr=5, ldh=5, p=one, h=one: lib.dbgsom_energy_rows(p, N, M, ldr, h, ldh, p, p, None)   # noqa: E731
    assert rows(M=0, ldr=0, ldh=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert rows(M=_native.MAX_PROTOTYPES + 1, ldr=20000, ldh=20000) == -1 and b"MAX_PROTOTYPES" in err()
    assert rows(ldr=4) == -1 and b"ldr" in err()
    assert rows(ldh=4) == -1 and b"ldh" in err()
    assert rows(N=-1) == -1 and b"shape" in err()
    assert rows(p=None) == -1 and b"null pointer" in err()
    assert rows(h=None) == -1 and b"null pointer" in err()
    assert rows(p=20) == -1 and b"aligned" in err()
    assert rows(h=20) == -1 and b"aligned" in err()
    assert rows(N=0, p=None, h=None) == 0   # no rows: nothing to do, nothing dereferenced

    need = lib.dbgsom_kneighbors_workspace_bytes(10, 5, 0)
    full = lambda dt=0, N=10, d=4, ldx=4, M=5, ldh=5, slab=0, p=one, h=one, w=one, ws=need: (   # noqa: E731
        lib.dbgsom_neighborhood_energy(p, dt, N, d, ldx, p, p, M, p, h, ldh, slab, p, p, w, ws, None))
    assert full(dt=7) == -1 and b"x_dtype" in err()
    assert full(ldx=3) == -1 and b"shape" in err()
    assert full(M=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert full(M=_native.MAX_PROTOTYPES + 1, ldh=20000) == -1 and b"MAX_PROTOTYPES" in err()
    assert full(ldh=4) == -1 and b"ldh" in err()
    assert full(slab=-1) == -1 and b"slab_rows" in err()
    assert full(p=None) == -1 and b"null pointer" in err()
    assert full(h=None) == -1 and b"null pointer" in err()
    assert full(w=None) == -1 and b"null pointer" in err()
    assert full(h=20) == -1 and b"aligned" in err()
    assert full(w=24) == -1 and b"16-byte aligned" in err()
    assert full(ws=need - 1) == -3 and (b"%d bytes, %d needed" % (need - 1, need)) in err()
    assert full(N=0, p=None, h=None, w=None, ws=0) == 0

    W, H = np.zeros((5, 4)), np.eye(5)
    out = np.zeros(64)
    w, h = W.ctypes.data, H.ctypes.data
    calls = (("dbgsom_ctx_distortion_query", lambda c, M, hh: (c, one, 0, 10, 4, w, M, hh, one, one)),
             ("dbgsom_ctx_distortion_query_device", lambda c, M, hh: (c, one, 0, 10, 4, 4, w, M, hh, one, one)),
             ("dbgsom_ctx_distortion_query_csr", lambda c, M, hh: (c, one, one, one, 0, 10, 4, 3, w, M, hh, one, one)))
    for name, args in calls:
        assert getattr(lib, name)(*args(None, 5, h)) == -1 and b"null context" in err()
        with pytest.raises(ValueError, match="null context"):
            _native.call(name, *args(None, 5, h))
        assert getattr(lib, name)(*args(out.ctypes.data, 0, h)) == -1 and b"MAX_PROTOTYPES" in err()   # (before the context is touched)
    assert lib.dbgsom_ctx_distortion_query_device(out.ctypes.data, one, 0, 10, 4, 3, w, 5, h, one, one) == -1 and b"ldx" in err()
