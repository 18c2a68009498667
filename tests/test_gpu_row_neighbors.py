"""MI355X: index_rows / row_neighbors -- scan_cells_kernel (csrc/row_neighbors.hip) through dbgsom_ctx_scan_cells_device
on crafted buffers against the oracle of tests/row_neighbors.py, bit for bit in idx and dist; the context calls (host rows
in chunks against rows in HBM, against the oracle fed with dbgsom_ctx_read_partition and dbgsom_ctx_kneighbors_query, the
DBGSOM_ESTATE refusals) and both estimators.  Results are prefilled with 0xFF bytes and lie between guard bytes.  No test
asserts on a clock."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import device_abi as da
from tests import golden_inputs as gi
from tests import row_neighbors as rn

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


@pytest.fixture(scope="module")
def be():
    from dbgsom_amd.backend import HipBackend

    b = HipBackend(0)
    yield b
    b.release()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    return np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])


class _Out:
    """Nq x k indices and distances, each the body of a GuardedWorkspace prefilled with 0xFF bytes"""

    def __init__(self, Nq, k):
        self.shape = (Nq, k)
        self.i, self.d = da.GuardedWorkspace(Nq * k * 8), da.GuardedWorkspace(Nq * k * 8)
        self.i.fill("ff")
        self.d.fill("ff")

    def read(self):
        """-> (dist, idx); the guard bytes around both must be intact"""
        assert self.i.intact() == (True, True) and self.d.intact() == (True, True), "a write outside the result"
        n = self.shape[0] * self.shape[1] * 8
        i = self.i.t.cpu().numpy()[self.i.off:self.i.off + n].view(np.int64).reshape(self.shape).copy()
        d = self.d.t.cpu().numpy()[self.d.off:self.d.off + n].view(np.float64).reshape(self.shape).copy()
        return d, i


def _scan_rc(nat, be, Xf, d, order, seg, M, Qf, probes, k, out=None, N=None):
    """the raw call on the full (padded) arrays Xf / Qf with ldx / ldq their widths -> (status, out)"""
    Xd, Qd, od, sd, pd = da.dev(Xf), da.dev(Qf), da.dev(order), da.dev(seg.view(np.int32)), da.dev(probes)
    Nq, n_probe = probes.shape
    out = out or _Out(Nq, k)
    rc = nat.load().dbgsom_ctx_scan_cells_device(
        be._ctx, Xd.data_ptr(), CODE[Xf.dtype], len(Xf) if N is None else N, d, Xf.shape[1], od.data_ptr(), sd.data_ptr(), M,
        Qd.data_ptr(), CODE[Qf.dtype], Nq, Qf.shape[1], pd.data_ptr(), n_probe, k, out.i.ptr, out.d.ptr)
    return rc, out


def _scan(nat, be, case, k=None):
    k = k or case["k"]
    rc, out = _scan_rc(nat, be, case["Xf"], case["d"], case["order"], case["seg"], case["M"], case["Qf"], case["probes"], k)
    assert rc == 0, nat.load().dbgsom_last_error()
    return out.read()


def _want(case, k=None):
    return rn.oracle(case["X"], case["winners"], case["probes"], case["Q"], k or case["k"])


# ---- 1. dbgsom_ctx_scan_cells_device on crafted buffers -------------------------------------------------------------
@pytest.mark.parametrize("d", rn.SCAN_D)
def test_scan_feature_counts(nat, be, d):
    case = rn.scan_case(d, 70, d, 5, pad=3)          # ldx, ldq = d + 3 with NaN in the padding
    assert _same(_scan(nat, be, case), _want(case))


def test_scan_refuses_wide_rows_with_a_status(nat, be):
    case = rn.scan_case(1, 4, 8, 2)
    Xf = np.zeros((case["Xf"].shape[0], 8193), dtype=np.float32)
    Qf = np.zeros((3, 8193), dtype=np.float32)
    rc, _ = _scan_rc(nat, be, Xf, 8193, case["order"], case["seg"], case["M"], Qf, case["probes"], 2)
    assert rc == EINVAL and b"8192" in nat.load().dbgsom_last_error()


@pytest.mark.parametrize("xt,qt", rn.DTYPES, ids=lambda t: np.dtype(t).name)
def test_scan_dtype_pairs(nat, be, xt, qt):
    case = rn.scan_case(3, 300, 65, 5, xt, qt, pad=1)
    assert _same(_scan(nat, be, case), _want(case))


@pytest.mark.parametrize("k", rn.SCAN_K)
def test_scan_neighbour_counts(nat, be, k):
    case = rn.scan_case(10 + k, 257, 20, k)
    assert _same(_scan(nat, be, case), _want(case))


@pytest.mark.parametrize("n_cand", rn.SCAN_COUNTS)
def test_scan_candidate_counts(nat, be, n_cand):
    case = rn.scan_case(20 + n_cand, n_cand, 33, 5, np.float64, np.float32, descending=n_cand % 2 == 1)
    got, want = _scan(nat, be, case), _want(case)
    assert _same(got, want)
    filled = min(5, n_cand)                            # fewer candidates than k: (inf, -1) behind them
    assert (got[1][0, :filled] >= 0).all() and (got[1][0, filled:] == -1).all() and np.isinf(got[0][0, filled:]).all()


@pytest.mark.parametrize("xt", [np.float32, np.float64], ids=["f32", "f64"])
def test_scan_duplicates_zero_and_non_finite_rows(nat, be, xt):
    case = rn.plant_specials(rn.scan_case(5, 400, 70, 8, xt, np.float64))
    case["Xf"] = np.ascontiguousarray(case["X"])
    got, want = _scan(nat, be, case), _want(case)
    assert _same(got, want)
    order, seg = case["order"], case["seg"]
    cand = np.concatenate([order[seg[0]:seg[1]], order[seg[2]:seg[3]]])
    assert got[0][0, 0] == 0.0 and got[1][0, 0] == cand[5]                          # the row equal to the query
    dup = sorted(int(r) for r in (cand[1], cand[67], cand[130], order[seg[3] - 1]))
    assert list(got[1][0, 1:5]) == dup and len(set(_bits(got[0][0, 1:5]))) == 1       # equal rho: the lower row first
    assert not set(int(r) for r in cand[7:10]) & set(int(i) for i in got[1][0])      # NaN, +inf, overflow: never listed
    assert np.isfinite(got[0][got[1] >= 0]).all()


def test_scan_only_non_finite_candidates_lists_nothing(nat, be):
    case = rn.scan_case(6, 5, 4, 3, np.float64, np.float64)
    rows = np.flatnonzero(np.isin(case["winners"], [0, 2]))
    case["X"][rows, 0] = [np.nan, np.inf, 1e200, -1e200, np.nan]
    case["Xf"] = np.ascontiguousarray(case["X"])
    got = _scan(nat, be, case)
    assert _same(got, _want(case)) and (got[1][0] == -1).all() and np.isinf(got[0][0]).all()


# ---- 2. the context calls -------------------------------------------------------------------------------------------
def _data(N, d, M, seed):
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(N, d)) + 2 * rng.integers(0, 5, size=(N, 1))).astype(np.float32)
    W = X[rng.choice(N, M, replace=False)].astype(np.float64) + 0.01
    Q = np.concatenate([X[rng.choice(N, 60)], rng.normal(size=(51, d)).astype(np.float32)])
    return X, W, Q


def _query_host(nat, be, Q, W, n_probe, k):
    idx, dist = np.full((len(Q), k), -7, dtype=np.int64), np.full((len(Q), k), -7.0)
    rc = nat.load().dbgsom_ctx_row_neighbors_query(be._ctx, Q.ctypes.data, CODE[Q.dtype], len(Q), Q.shape[1], W.ctypes.data,
                                                   len(W), n_probe, k, idx.ctypes.data, dist.ctypes.data)
    return rc, (dist, idx)


@pytest.mark.parametrize("d,M", [(20, 25), (784, 25), (20, 300), (784, 300)])
def test_context_host_chunks_device_rows_and_oracle(nat, be, d, M):
    N, k, n_probe = 3000, 7, 5
    X, W, Q = _data(N, d, M, d + M)
    be.load(X)
    try:
        _, winners = be.partition(W, want_winners=True)
        order, seg = be.read_partition()
        assert np.array_equal(np.sort(order), np.arange(N)) and seg[0] == 0 and seg[M] == N
        for j in (0, M // 2, M - 1):
            assert np.array_equal(order[seg[j]:seg[j + 1]], np.flatnonzero(winners == j))
        probes = be.kneighbors(W, n_probe, Q)[1]
        want = rn.oracle(X, winners, probes, Q, k)
        be.distances_chunk_rows = 37
        try:
            rc, host = _query_host(nat, be, Q, W, n_probe, k)
        finally:
            be.distances_chunk_rows = 0
        assert rc == 0, nat.load().dbgsom_last_error()
        out = _Out(len(Q), k)
        Qd = da.dev(Q)
        rc = nat.load().dbgsom_ctx_row_neighbors_query_device(be._ctx, Qd.data_ptr(), CODE[Q.dtype], len(Q), d, d,
                                                              W.ctypes.data, M, n_probe, k, out.i.ptr, out.d.ptr)
        assert rc == 0, nat.load().dbgsom_last_error()
        assert _same(host, want) and _same(out.read(), want)
        assert _same(be.row_neighbors(W, k, n_probe, Q), want)
    finally:
        be.release()


def test_context_state_refusals(nat, be):
    X, W, Q = _data(300, 20, 25, 1)
    lib = nat.load()
    be.load(X)
    try:
        assert _query_host(nat, be, Q, W, 3, 2)[0] == ESTATE and b"partition" in lib.dbgsom_last_error()
        assert lib.dbgsom_ctx_read_partition(be._ctx, None, None) == ESTATE
        be.partition(W)
        assert _query_host(nat, be, Q, W, 3, 2)[0] == 0
        assert _query_host(nat, be, Q, W[:24], 3, 2)[0] == ESTATE and b"M is not" in lib.dbgsom_last_error()
        assert _query_host(nat, be, Q[:, :19].copy(), W[:, :19].copy(), 3, 2)[0] == EINVAL
        be.load(X)                                                       # a reload drops the partition
        assert _query_host(nat, be, Q, W, 3, 2)[0] == ESTATE
        with pytest.raises(ValueError, match="partition"):
            be.row_neighbors(W, 2, 3, Q)
    finally:
        be.release()
    below = be.csr_densify_below
    be.csr_densify_below = 0                                             # (rows of 20 features stay CSR residents)
    try:
        be.load(sp.csr_matrix(X))
        assert be.resident_csr
        be.partition(W)
        assert _query_host(nat, be, Q, W, 3, 2)[0] == ESTATE and b"CSR" in lib.dbgsom_last_error()
        be.load(X, storage="bf16")
        be.partition(W)
        assert _query_host(nat, be, Q, W, 3, 2)[0] == ESTATE and b"bfloat16" in lib.dbgsom_last_error()
    finally:
        be.csr_densify_below = below
        be.release()


# ---- 3. the estimators ----------------------------------------------------------------------------------------------
KW = dict(random_state=0, n_iter=12)


@pytest.fixture(scope="module", params=["vq", "clf"])
def fitted(request):
    from dbgsom_amd import SomClassifier, SomVQ

    X = np.ascontiguousarray(gi.case_X("digits_f64")[0][:900], dtype=np.float32)
    y = None if request.param == "vq" else gi.case_X("digits_clf")[1][:900]
    est = SomVQ(**KW).fit(X) if y is None else SomClassifier(**KW).fit(X, y)
    return est, X, y


def test_estimator_host_array_against_tensor_and_invariants(fitted):
    import torch

    est, X, y = fitted
    est.index_rows(X)
    M = len(est.weights_)
    assert est.n_indexed_ == len(X) and est.index_counts_.sum() == len(X) and est.index_counts_.shape == (M,)
    rows = np.arange(0, len(X), 7)
    Q = X[rows]
    engine = est._engine()
    before = engine.sample_traffic()
    dist, idx = est.row_neighbors(Q, 6, min(4, M))
    after = engine.sample_traffic()
    assert after["x_download_bytes"] - before["x_download_bytes"] == len(Q) * 6 * 16
    assert after["x_upload_bytes"] - before["x_upload_bytes"] == Q.nbytes
    assert dist.dtype == np.float64 and idx.dtype == np.int64 and dist.shape == idx.shape == (len(Q), 6)
    Qt = torch.from_numpy(Q).cuda()
    before = engine.sample_traffic()
    dt, it = est.row_neighbors(Qt, 6, min(4, M))
    assert engine.sample_traffic() == before                     # nothing of Q or the results crosses PCIe
    assert dt.is_cuda and it.is_cuda
    assert _same((dt.cpu().numpy(), it.cpu().numpy()), (dist, idx))
    # a row of X finds itself (or an identical row with a lower number) at distance 0
    assert (dist[:, 0] == 0).all() and (idx[:, 0] <= rows).all()
    assert all(np.array_equal(X[i], X[r]) for i, r in zip(idx[:, 0], rows))
    # every listed row's unit is among the query's nearest units
    units = est.kneighbors(Q, min(4, M), return_distance=False)
    unit_of = est.kneighbors(X, 1, return_distance=False)[:, 0]
    for q in range(len(Q)):
        listed = idx[q][idx[q] >= 0]
        assert np.isin(unit_of[listed], units[q]).all()
    # fewer probes: candidates are a subset, so no listed distance gets smaller
    d1 = est.row_neighbors(Q, 6, 1)[0]
    assert (d1 >= dist).all()
    # tensor index: the same bits
    est.index_rows(torch.from_numpy(X).cuda())
    assert _same(est.row_neighbors(Q, 6, min(4, M)), (dist, idx))


def test_estimator_all_units_is_the_exact_search(fitted):
    est, X, y = fitted
    M = len(est.weights_)
    assert M <= 32                                               # (a map this small probes every unit)
    est.index_rows(X)
    rng = np.random.default_rng(3)
    Q = (X[rng.choice(len(X), 40)] + rng.normal(size=(40, X.shape[1])).astype(np.float32))
    dist, idx = est.row_neighbors(Q, 10, M)
    D2 = ((Q.astype(np.longdouble)[:, None, :] - X.astype(np.longdouble)[None, :, :]) ** 2).sum(axis=2)
    want = np.sort(D2, axis=1)[:, :10]
    assert (idx >= 0).all()
    assert (np.abs(dist.astype(np.longdouble) ** 2 - want) <= (rn.rho_bound(X.shape[1]) + 2 * rn.U) * want).all()


def test_estimator_refusals_after_fit_and_pickle(fitted):
    import pickle

    from sklearn.base import clone

    est, X, y = fitted
    est.index_rows(X)
    other = pickle.loads(pickle.dumps(est))
    with pytest.raises(ValueError, match="index_rows"):
        other.row_neighbors(X[:2], 2, 2)
    with pytest.raises(TypeError, match="dense"):
        est.row_neighbors(sp.csr_matrix(X[:2]), 2, 2)
    est._engine().load(X)                                        # someone else replaced the resident rows
    with pytest.raises(ValueError, match="replaced"):
        est.row_neighbors(X[:2], 2, 2)
    again = clone(est).fit(X[:300], None if y is None else y[:300])
    with pytest.raises(ValueError, match="index_rows"):
        again.row_neighbors(X[:2], 2, 2)
    again.index_rows(X[:300])
    again.fit(X[:300], None if y is None else y[:300])           # a later fit drops the index
    with pytest.raises(ValueError, match="index_rows"):
        again.row_neighbors(X[:2], 2, 2)
