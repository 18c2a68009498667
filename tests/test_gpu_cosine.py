"""MI355X: ``metric="cosine"`` (csrc/cosine.hip, the cosine forms of the MFMA kernels, the cosine context calls) against
the NumPy restatement of tests/cosine.py -- raw device-level calls bit for bit (index and distance) over the shape table
of the distance matrix, the context calls, one epoch against the stand-in's, and the estimators on ``HipBackend`` against
the stand-in."""
import numpy as np
import pytest

from tests import cosine as cs
from tests import device_abi as da
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu

# new prototypes, errors and change of an epoch against the oracle: tests/test_gpu_manhattan.py
W_RTOL, W_ATOL, E_RTOL, CHG_REL = 1e-11, 1e-13, 1e-12, 1e-9
# weights_ of a whole fit, device against CPU: tests/test_gpu_manhattan.py
FIT_RTOL, FIT_ATOL = 1e-8, 1e-10
SENTINEL = -77.0


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


def _sync():
    import torch

    torch.cuda.synchronize()


def _full(n, value, dtype):
    import torch

    return torch.full((int(n),), value, dtype=getattr(torch, dtype), device="cuda")


class Staged:
    """X (as stored) with rows ldx apart, row 0 x_off elements into its allocation, and W (float64, contiguous) on the
    device, NaN in the padding; u and v made there by dbgsom_row_sqnorms and dbgsom_inv_norms"""

    def __init__(self, nat, X, W, xpad=0, x_off=0):
        self.dtype = "f32" if X.dtype == np.float32 else "f64"
        self.N, self.d = X.shape
        self.M = W.shape[0]
        self.ldx = self.d + xpad
        self.xt, self.x = da.stage(np.ascontiguousarray(X), self.ldx, x_off, self.dtype)
        self.wt, self.w = da.stage(np.ascontiguousarray(W, dtype=np.float64), self.d, 0, "f64")
        self.xx, self.ww = _full(self.N, SENTINEL, "float64"), _full(self.M, SENTINEL, "float64")
        self.ut, self.vt = _full(self.N, SENTINEL, "float64"), _full(self.M, SENTINEL, "float64")
        nat.call("dbgsom_row_sqnorms", self.x, da.CODE[self.dtype], self.N, self.d, self.ldx, self.xx.data_ptr(), da.stream())
        nat.call("dbgsom_row_sqnorms", self.w, da.CODE["f64"], self.M, self.d, self.d, self.ww.data_ptr(), da.stream())
        nat.call("dbgsom_inv_norms", self.xx.data_ptr(), self.N, self.ut.data_ptr(), da.stream())
        nat.call("dbgsom_inv_norms", self.ww.data_ptr(), self.M, self.vt.data_ptr(), da.stream())
        self.u, self.v = self.ut.data_ptr(), self.vt.data_ptr()


def raw_bmu(nat, s, k):
    """dbgsom_bmu_cosine -> (dist, idx), (N, k), with sentinels around both checked"""
    idx, dist = _full((s.N + 2) * k, -77, "int64"), _full((s.N + 2) * k, SENTINEL, "float64")
    nat.call("dbgsom_bmu_cosine", s.x, da.CODE[s.dtype], s.N, s.d, s.ldx, s.u, s.w, s.M, s.v, k, idx.data_ptr() + 8 * k,
             dist.data_ptr() + 8 * k, da.stream())
    _sync()
    idx, dist = idx.cpu().numpy().reshape(s.N + 2, k), dist.cpu().numpy().reshape(s.N + 2, k)
    assert (idx[[0, -1]] == -77).all() and (dist[[0, -1]] == SENTINEL).all()
    return dist[1:-1], idx[1:-1]


def raw_distances(nat, s, ldo=None, off=0):
    """dbgsom_distances_cosine into a buffer of sentinels with row 0 `off` elements in -> (N, M), everything outside
    the result checked to be untouched"""
    ldo = s.M if ldo is None else ldo
    out = _full(off + s.N * ldo + 4, SENTINEL, "float64")
    assert out.data_ptr() % 256 == 0
    nat.call("dbgsom_distances_cosine", s.x, da.CODE[s.dtype], s.N, s.d, s.ldx, s.u, s.w, s.M, s.v, out.data_ptr() + 8 * off,
             ldo, da.stream())
    _sync()
    flat = out.cpu().numpy()
    body = flat[off:off + s.N * ldo].reshape(s.N, ldo)
    assert (flat[:off] == SENTINEL).all() and (flat[off + s.N * ldo:] == SENTINEL).all() and (body[:, s.M:] == SENTINEL).all()
    return body[:, :s.M]


def raw_kneighbors(nat, s, k, slab_rows=0, short=False):
    lib = nat.load()
    nbytes = lib.dbgsom_kneighbors_cosine_workspace_bytes(s.N, s.M, slab_rows)
    ws_t, ws = da.workspace(nbytes)
    idx, dist = _full((s.N + 2) * k, -77, "int64"), _full((s.N + 2) * k, SENTINEL, "float64")
    args = (s.x, da.CODE[s.dtype], s.N, s.d, s.ldx, s.u, s.w, s.M, s.v, k, slab_rows, idx.data_ptr() + 8 * k,
            dist.data_ptr() + 8 * k, ws)
    if short:
        rc = lib.dbgsom_kneighbors_cosine(*args, nbytes - 256, da.stream())
        _sync()
        assert (idx == -77).all() and (dist == SENTINEL).all()                  # nothing was launched
        return rc
    nat.call("dbgsom_kneighbors_cosine", *args, nbytes, da.stream())
    _sync()
    idx, dist = idx.cpu().numpy().reshape(s.N + 2, k), dist.cpu().numpy().reshape(s.N + 2, k)
    assert (idx[[0, -1]] == -77).all() and (dist[[0, -1]] == SENTINEL).all()
    return dist[1:-1], idx[1:-1]


# ---- 1. device level --------------------------------------------------------------------------------------------------
def test_inv_norms_raw(nat):
    import torch

    t = np.array([0.0, 5e-324, 2.2e-308, 1e-300, 0.25, 1.0, 2.0, 3.0, 1e300, np.inf, np.nan, -0.0, -1.0]
                 + list(np.random.default_rng(0).uniform(1e-6, 1e6, 500)))
    src = torch.from_numpy(t).cuda()
    out = _full(len(t) + 2, SENTINEL, "float64")
    nat.call("dbgsom_inv_norms", src.data_ptr(), len(t), out.data_ptr() + 8, da.stream())
    _sync()
    got = out.cpu().numpy()
    assert got[0] == SENTINEL and got[-1] == SENTINEL
    want = cs.inv_norms(t)
    assert np.array_equal(got[1:-1], want, equal_nan=True)                      # sqrt, then the division: two roundings
    assert got[1] == 0.0 and got[12] == 0.0 and np.isfinite(got[2]) and np.isnan(got[[10, 11, 13]]).all()


@pytest.mark.parametrize("case", cs.CASES, ids=cs.CASE_IDS)
def test_search_and_matrix_bit_for_bit(nat, case):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, C = cs.case_data(case)
    s = Staged(nat, X, W, pad, x_off)
    _sync()
    assert np.array_equal(s.ut.cpu().numpy(), cs.inv_norms(cs.sqnorm_chain(X)))
    assert np.array_equal(s.vt.cpu().numpy(), cs.inv_norms(cs.sqnorm_chain(W)))
    got = raw_distances(nat, s, ldo=M + ldo_pad, off=out_off)
    assert np.array_equal(got, C)
    for k in (1, 2):
        if k > M:
            continue
        dist, idx = raw_bmu(nat, s, k)
        want_dist, want_idx = cs.select(C, k)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
        if k == 1:                                                               # the matrix's row minimum is the search's output
            assert np.array_equal(got.min(axis=1), dist[:, 0]) and np.array_equal(got.argmin(axis=1), idx[:, 0])
    if N >= 3:
        assert (got[0] == 1.0).all() and idx[0, 0] == 0                          # the zero row: 1 from everything, lowest index
    if M >= 4:
        assert np.array_equal(got[:, 0], got[:, M - 1])                          # the duplicated prototype: same bits


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("d", [6, 16])
def test_edge_rows(nat, dtype, d):
    rng = np.random.default_rng(2)
    M = 70
    W = rng.normal(size=(M, d)).astype(np.float32).astype(np.float64)
    W[60] = W[14]
    W[30] = 4.0 * W[14]                                                         # collinear
    W[5] = 0.0                                                                  # a zero prototype
    X = rng.normal(size=(130, d)).astype(np.float32).astype(np.float64)
    X[0] = W[7]
    X[1] = -W[7]
    X[2, 3] = np.nan
    X[3, 0] = np.inf
    X[4] = 0.0
    X[5, 5] = -np.inf
    if dtype == "f64":
        X[6, 2] = 1e200                                                         # the squared norm overflows
        X[7] = 1e-200                                                           # ... underflows to 0
    X = X.astype(cs.NP_DTYPE[dtype])
    C = cs.cosine_distances(X, W)                                               # (float64: 1e200 needs the emulation)
    s = Staged(nat, X, W, 16 if d == 16 else 1, 0)
    got = raw_distances(nat, s)
    assert np.array_equal(got, C, equal_nan=True)
    assert np.isnan(got[[2, 3, 5]]).all() and (got[4] == 1.0).all() and (got[:, 5][[0, 1, 8]] == 1.0).all()
    assert got[0, 7] <= 2 * cs.U and got[1, 7] >= 2.0 - 2 * cs.U
    bad = [2, 3, 5] + ([6] if dtype == "f64" else [])
    if dtype == "f64":
        assert np.isnan(got[6]).all() and (got[7] == 1.0).all()
    for k in (1, 2):
        dist, idx = raw_bmu(nat, s, k)
        want_dist, want_idx = cs.select(C, k)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
        for r in bad:                                                            # NaN / infinity / overflow: nothing wins
            assert (idx[r] == -1).all() and np.isinf(dist[r]).all()
        assert idx[4].tolist() == [0, 1][:k]                                     # the zero row: the lowest indices
    dist, idx = raw_kneighbors(nat, s, 8)
    want_dist, want_idx = cs.select(C, 8)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
    assert (idx[bad] == -1).all()


@pytest.mark.parametrize("case", [c for c in cs.CASES if (c[1], c[2]) in ((300, 5), (300, 33), (300, 260), (300, 31), (127, 260),
                                                                       (129, 64), (300, 1), (1, 260))],
                         ids=lambda c: "%s-N%d-M%d-d%d-pad%d" % c[:5])
def test_kneighbors_against_the_oracle(nat, case):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, C = cs.case_data(case)
    s = Staged(nat, X, W, pad, x_off)
    for k in (1, 2, 8, 32):
        if k > M:
            continue
        want_dist, want_idx = cs.select(C, k)                                    # a stable sort on (c, j)
        one_d, one_i = raw_kneighbors(nat, s, k)
        assert np.array_equal(one_i, want_idx) and np.array_equal(one_d, want_dist)
        if N == 300:
            three_d, three_i = raw_kneighbors(nat, s, k, slab_rows=128)          # three slabs against one
            assert np.array_equal(three_i, one_i) and np.array_equal(three_d, one_d)
    assert raw_kneighbors(nat, s, 1, short=True) == -3
    assert b"workspace of" in nat.load().dbgsom_last_error()


# ---- 2. the context calls ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backend():
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0)
    yield be
    be.release()


QUERY_CASES = [c for c in cs.CASES if c[:4] in (("f32", 300, 33, 784), ("f64", 300, 31, 48), ("f32", 300, 260, 17))]


@pytest.mark.parametrize("case", QUERY_CASES, ids=lambda c: "%s-N%d-M%d-d%d" % c[:4])
def test_queries_in_chunks_and_from_device_rows(backend, case):
    import torch

    be = backend
    dtype, N, M, d = case[:4]
    X, W, C = cs.case_data(case)
    before = be.sample_traffic()
    one = (be.bmu_cosine(W, 2, X), be.distances_cosine(W, X), be.kneighbors_cosine(W, 5, X))
    moved = be.sample_traffic()
    assert moved["x_upload_bytes"] - before["x_upload_bytes"] == 3 * X.nbytes
    assert moved["x_download_bytes"] - before["x_download_bytes"] == N * (2 * 16 + M * 8 + 5 * 16)
    want2, want5 = cs.select(C, 2), cs.select(C, 5)
    assert np.array_equal(one[0][0], want2[0]) and np.array_equal(one[0][1], want2[1])
    assert np.array_equal(one[1], C)
    assert np.array_equal(one[2][0], want5[0]) and np.array_equal(one[2][1], want5[1])
    d1, i1 = be.bmu_cosine(W, 1, X)
    assert d1.shape == (N,) and np.array_equal(i1, want2[1][:, 0]) and np.array_equal(d1, want2[0][:, 0])
    keep = (be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows)
    try:                                                                         # several host chunks against one
        be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows = 64, 50, 16
        many = (be.bmu_cosine(W, 2, X), be.distances_cosine(W, X), be.kneighbors_cosine(W, 5, X))
        xt = torch.from_numpy(np.array(X)).cuda()
        wide = torch.full((N, d + 3), float("nan"), dtype=xt.dtype, device="cuda")
        wide[:, :d] = xt
        for rows in (xt, wide[:, :d]):                                           # device rows, contiguous and strided
            now = be.sample_traffic()
            dev = (be.bmu_cosine(W, 2, rows), be.distances_cosine(W, rows), be.kneighbors_cosine(W, 5, rows))
            assert be.sample_traffic() == now                                    # no bytes of X are counted up
            assert all(t.is_cuda for t in (dev[0][0], dev[0][1], dev[1], dev[2][0], dev[2][1]))
            dev = ((dev[0][0].cpu().numpy(), dev[0][1].cpu().numpy()), dev[1].cpu().numpy(),
                   (dev[2][0].cpu().numpy(), dev[2][1].cpu().numpy()))
            for got in (many, dev):
                assert np.array_equal(got[0][0], one[0][0]) and np.array_equal(got[0][1], one[0][1])
                assert np.array_equal(got[1], one[1])
                assert np.array_equal(got[2][0], one[2][0]) and np.array_equal(got[2][1], one[2][1])
    finally:
        be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows = keep


@pytest.mark.parametrize("case", QUERY_CASES[:2], ids=lambda c: "%s-N%d-M%d-d%d" % c[:4])
def test_the_resident_search(backend, case):
    X, W, C = cs.case_data(case)
    be = backend.load(np.array(X))
    try:
        be.set_metric("cosine")
        for k in (1, 2):
            dist, idx = be.bmu(W, k)
            want_dist, want_idx = cs.select(C, k)
            assert np.array_equal(np.reshape(idx, (-1, k)), want_idx) and np.array_equal(np.reshape(dist, (-1, k)), want_dist)
        assert np.array_equal(be.resident_winners(W), cs.select(C, 1)[1][:, 0])
        assert be.quantization_error(W) == float(np.mean(cs.select(C, 1)[0][:, 0]))
    finally:
        be.release()
    assert be._metric == "euclidean"


def test_context_argument_errors_are_status_codes(backend, nat):
    lib = nat.load()
    be = backend
    X, W, _ = cs.case_data(("f64", 127, 31, 17, 0, 0, 0, 0))
    X, W = np.ascontiguousarray(X), np.ascontiguousarray(W)
    N, d, M = 127, 17, 31
    idx, dist = np.full((N, 2), -5, dtype=np.int64), np.full((N, 2), -5.0)
    args = (X.ctypes.data, 1, N, d, W.ctypes.data, M)
    err = lib.dbgsom_last_error
    assert lib.dbgsom_ctx_bmu_query_cosine(be._ctx, X.ctypes.data, 2, N, d, W.ctypes.data, M, 1, idx.ctypes.data,
                                           dist.ctypes.data) == -1 and b"x_dtype" in err()          # no bfloat16 rows
    assert lib.dbgsom_ctx_bmu_query_cosine(be._ctx, *args, 3, idx.ctypes.data, dist.ctypes.data) == -1 and b"k must" in err()
    assert lib.dbgsom_ctx_bmu_query_cosine(be._ctx, *args, 1, None, dist.ctypes.data) == -1 and b"null" in err()
    assert lib.dbgsom_ctx_kneighbors_query_cosine(be._ctx, *args, 32, idx.ctypes.data, dist.ctypes.data) == -1 and b"k <= M" in err()
    assert lib.dbgsom_ctx_distances_query_cosine(be._ctx, *args, None) == -1 and b"null" in err()
    assert lib.dbgsom_ctx_distances_query_cosine_device(be._ctx, 8, 1, N, d, d - 1, W.ctypes.data, M, 8, M) == -1   # ldx < d
    assert lib.dbgsom_ctx_distances_query_cosine_device(be._ctx, 8, 1, N, d, d, W.ctypes.data, M, 8, M - 1) == -1 and b"ldo" in err()
    assert (idx == -5).all() and (dist == -5.0).all()                            # nothing was launched
    assert lib.dbgsom_ctx_bmu_cosine(be._ctx, W.ctypes.data, M, 1, idx.ctypes.data, dist.ctypes.data) == -4      # no rows loaded
    be.load(np.ascontiguousarray(X, dtype=np.float32), storage="bf16")
    try:
        with pytest.raises(ValueError, match="bfloat16"):
            nat.call("dbgsom_ctx_bmu_cosine", be._ctx, W.ctypes.data, M, 1, idx.ctypes.data, dist.ctypes.data)
    finally:
        be.release()
    be.load(X)
    try:
        be.set_sample_weight(np.ones(N))
        with pytest.raises(ValueError, match="sample weights"):
            nat.call("dbgsom_ctx_bmu_cosine", be._ctx, W.ctypes.data, M, 1, idx.ctypes.data, dist.ctypes.data)
        be.set_sample_weight(None)
        be.set_metric("cosine")
        out = np.empty((M, d))                                                   # the epoch before set_topology
        rc = lib.dbgsom_ctx_epoch_cosine(be._ctx, W.ctypes.data, M, 0.1, 1.0, 0, out.ctypes.data, dist.ctypes.data,
                                         dist.ctypes.data, dist.ctypes.data, None, None)
        assert rc == -4 and b"topology" in err()
    finally:
        be.release()
    import scipy.sparse as sp

    keep = be.csr_densify_below
    be.csr_densify_below = 0                                                     # CSR residents (0: never densified)
    try:
        be.load(sp.csr_matrix(X))
        with pytest.raises(ValueError, match="CSR"):
            nat.call("dbgsom_ctx_bmu_cosine", be._ctx, W.ctypes.data, M, 1, idx.ctypes.data, dist.ctypes.data)
    finally:
        be.release()
        be.csr_densify_below = keep


# ---- 3. one epoch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["compact", "aligned"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_epoch_against_the_stand_in(backend, dtype, layout):
    N, d, M = 300, 16, 9
    X, _ = cs.angular_blobs()
    X = np.asarray(X[:N], dtype=cs.NP_DTYPE[dtype])
    rng = np.random.default_rng(9)
    W = (np.asarray(X[rng.choice(N, M, replace=False)], dtype=np.float64) + 0.1 * rng.normal(size=(M, d)))
    W = W.astype(np.float32).astype(np.float64)                                  # the oracle's plain form applies
    if dtype == "f64":
        X = X.astype(np.float32).astype(np.float64)
    hop = gi.lattice_hops(3, 3)
    sigma, gamma = 1.4, float(np.var(X, axis=0).sum() ** -1)
    ref_be = cs.CosineOracleBackend().load(X)
    ref_be.set_metric("cosine")
    ref = ref_be.epoch_cosine(W, hop, sigma, gamma, layout, want_assignments=True)
    be = backend.load(X)
    try:
        be.set_metric("cosine")
        res = be.epoch_cosine(W, hop, sigma, gamma, layout, want_assignments=True)
        assert np.array_equal(res.winners, ref.winners) and np.array_equal(res.distances, ref.distances)
        np.testing.assert_allclose(res.new_weights, ref.new_weights, rtol=W_RTOL, atol=W_ATOL)
        np.testing.assert_allclose(res.errors, ref.errors, rtol=E_RTOL)
        assert np.array_equal(res.activations, ref.activations)
        assert res.change_total == pytest.approx(ref.change_total, rel=CHG_REL)
        held = be._get("device_bytes")
        again = be.epoch_cosine(W, hop, sigma, gamma, layout, want_assignments=True)
        assert be._get("device_bytes") == held                                   # u stays, nothing grows between two epochs
        assert np.array_equal(again.winners, res.winners) and np.array_equal(again.distances, res.distances)
        assert be.quantization_error(W) == float(np.mean(ref.distances))          # a host mean of the same bits
        with pytest.raises(ValueError, match="resident"):
            from dbgsom_amd.backend import RESIDENT
            be.epoch_cosine(RESIDENT, hop, sigma, gamma, layout)
    finally:
        be.release()


def test_u_of_the_resident_rows_belongs_to_the_context(backend):
    """u is a buffer of the context like the others: counted in "device_bytes" (the list dbgsom_ctx_destroy frees)"""
    N, d, M = 200000, 16, 4
    X = np.ones((N, d), dtype=np.float32)
    W = np.ones((M, d))
    be = backend.load(X)
    try:
        be.set_metric("cosine")
        before = be._get("device_bytes")
        dist, idx = be.bmu(W, 1)
        assert (idx == 0).all() and (dist == 0.0).all()                          # 16 * (1/4) * (1/4): exact
        assert be._get("device_bytes") - before >= N * 8
    finally:
        be.release()


# ---- 4. the estimators ------------------------------------------------------------------------------------------------
def _fit_pair(cls, backend, **kw):
    X, lab = cs.angular_blobs()
    args = (X, lab) if cls.__name__ == "SomClassifier" else (X,)
    gpu = cls(backend=backend, metric="cosine", **cs.FIT_KW, **kw).fit(*args)
    cpu = cls(backend=cs.CosineOracleBackend(), metric="cosine", **cs.FIT_KW, **kw).fit(*args)
    return gpu, cpu, X, lab


def test_somvq_on_the_device_against_the_stand_in(backend):
    import torch
    from dbgsom_amd import SomVQ

    X, _ = cs.angular_blobs()
    eu_before = SomVQ(backend=backend, **cs.FIT_KW).fit(X)
    gpu, cpu, X, _ = _fit_pair(SomVQ, backend)
    assert len(gpu.weights_) == len(cpu.weights_) > 4 and np.array_equal(gpu.labels_, cpu.labels_)
    np.testing.assert_allclose(gpu.weights_, cpu.weights_, rtol=FIT_RTOL, atol=FIT_ATOL)
    assert gpu.quantization_error_ == pytest.approx(cpu.quantization_error_, rel=FIT_RTOL)
    assert gpu.topographic_error_ == cpu.topographic_error_
    assert np.array_equal(gpu.predict(X), gpu.labels_)
    C = gpu.prototype_distances(X)
    assert np.array_equal(C, cs.cosine_distances(X, gpu.weights_))
    k = min(5, len(gpu.weights_))
    dist, idx = gpu.kneighbors(X, n_neighbors=k)
    assert np.array_equal(idx[:, 0], gpu.predict(X)) and np.array_equal(dist, np.take_along_axis(C, idx, axis=1))
    assert gpu.calculate_quantization_error(X) == pytest.approx(float(np.mean(C.min(axis=1))), rel=1e-15)
    xt = torch.from_numpy(np.array(X)).cuda()                                     # the same queries from a tensor
    td, ti = gpu.kneighbors(xt, n_neighbors=k)
    assert td.is_cuda and ti.is_cuda and gpu.predict(xt).is_cuda and gpu.prototype_distances(xt).is_cuda
    assert np.array_equal(td.cpu().numpy(), dist) and np.array_equal(ti.cpu().numpy(), idx)
    assert np.array_equal(gpu.predict(xt).cpu().numpy(), gpu.labels_)
    assert np.array_equal(gpu.prototype_distances(xt).cpu().numpy(), C)
    assert gpu.calculate_quantization_error(xt) == gpu.calculate_quantization_error(X)
    from_tensor = SomVQ(backend=backend, metric="cosine", **cs.FIT_KW).fit(xt)
    assert np.array_equal(from_tensor.weights_, gpu.weights_)                     # the fit on rows that live in HBM
    assert np.array_equal(from_tensor.labels_, gpu.labels_)
    eu_after = SomVQ(backend=backend, **cs.FIT_KW).fit(X)
    assert np.array_equal(eu_before.weights_, eu_after.weights_) and np.array_equal(eu_before.labels_, eu_after.labels_)
    assert not np.array_equal(eu_after.labels_, gpu.labels_) or not np.array_equal(eu_after.weights_, gpu.weights_)


def test_classifier_on_the_device_against_the_stand_in(backend):
    from dbgsom_amd import SomClassifier

    gpu, cpu, X, lab = _fit_pair(SomClassifier, backend)
    assert len(gpu.weights_) == len(cpu.weights_)
    np.testing.assert_allclose(gpu.weights_, cpu.weights_, rtol=FIT_RTOL, atol=FIT_ATOL)
    labels = lambda est: [est.som_.nodes[n]["label"] for n in est.neurons_]
    assert labels(gpu) == labels(cpu)
    assert np.array_equal(gpu.predict(X), cpu.predict(X))
