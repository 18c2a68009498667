"""MI355X: ``metric="manhattan"`` (csrc/manhattan.hip, the Manhattan context calls) against the NumPy restatement of
tests/manhattan.py -- raw device-level calls bit for bit (index and distance) at the shapes where the kernels can go
wrong, the context calls, one epoch against the stand-in's, and the estimators on ``HipBackend`` against the stand-in."""
import numpy as np
import pytest

from tests import device_abi as da
from tests import golden_inputs as gi
from tests import manhattan as mh

pytestmark = pytest.mark.gpu

# new prototypes, errors and change of an epoch against the oracle: tests/test_gpu_parity.py, tests/test_gpu_masked_fit.py
W_RTOL, W_ATOL, E_RTOL, CHG_REL = 1e-11, 1e-13, 1e-12, 1e-9
# weights_ of a whole fit, device against CPU: tests/test_gpu_estimator.py, tests/test_gpu_csr.py
FIT_RTOL, FIT_ATOL = 1e-8, 1e-10


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
    """X (as stored) with rows ldx apart and W (float64) with rows ldw apart on the device, NaN in the padding"""

    def __init__(self, X, W, xpad=0, wpad=0):
        self.dtype = "f32" if X.dtype == np.float32 else "f64"
        self.N, self.d = X.shape
        self.M = W.shape[0]
        self.ldx, self.ldw = self.d + xpad, self.d + wpad
        self.xt, self.x = da.stage(np.ascontiguousarray(X), self.ldx, 0, self.dtype)
        self.wt, self.w = da.stage(np.ascontiguousarray(W, dtype=np.float64), self.ldw, 0, "f64")


def raw_bmu(nat, s, k, n=None, row0=0):
    """dbgsom_bmu_manhattan on rows row0 .. row0 + n -> (dist, idx), (n, k), with sentinels around both checked"""
    lib = nat.load()
    n = s.N if n is None else n
    nbytes = lib.dbgsom_bmu_manhattan_workspace_bytes(da.CODE[s.dtype], n, s.d, s.M)
    ws_t, ws = da.workspace(nbytes)
    idx, dist = _full((n + 2) * k, -77, "int64"), _full((n + 2) * k, -77.0, "float64")
    nat.call("dbgsom_bmu_manhattan", s.x + row0 * s.ldx * da.ITEM[s.dtype], da.CODE[s.dtype], n, s.d, s.ldx, s.w, s.M, s.ldw,
             k, idx.data_ptr() + 8 * k, dist.data_ptr() + 8 * k, ws, nbytes, da.stream())
    _sync()
    idx, dist = idx.cpu().numpy().reshape(n + 2, k), dist.cpu().numpy().reshape(n + 2, k)
    assert (idx[[0, -1]] == -77).all() and (dist[[0, -1]] == -77.0).all()
    return dist[1:-1], idx[1:-1]


def raw_distances(nat, s, ldo=None, off=0):
    """dbgsom_distances_manhattan into a buffer of -77 with row 0 `off` elements in -> (N, ldo) with everything
    outside the result checked to be untouched"""
    lib = nat.load()
    ldo = s.M if ldo is None else ldo
    nbytes = lib.dbgsom_bmu_manhattan_workspace_bytes(da.CODE[s.dtype], s.N, s.d, s.M)
    ws_t, ws = da.workspace(nbytes)
    out = _full(off + s.N * ldo + 4, -77.0, "float64")
    assert out.data_ptr() % 256 == 0
    nat.call("dbgsom_distances_manhattan", s.x, da.CODE[s.dtype], s.N, s.d, s.ldx, s.w, s.M, s.ldw, out.data_ptr() + 8 * off,
             ldo, ws, nbytes, da.stream())
    _sync()
    flat = out.cpu().numpy()
    body = flat[off:off + s.N * ldo].reshape(s.N, ldo)
    assert (flat[:off] == -77.0).all() and (flat[off + s.N * ldo:] == -77.0).all() and (body[:, s.M:] == -77.0).all()
    return body[:, :s.M]


def raw_kneighbors(nat, s, k, slab_rows=0):
    lib = nat.load()
    nbytes = lib.dbgsom_kneighbors_manhattan_workspace_bytes(da.CODE[s.dtype], s.N, s.d, s.M, slab_rows)
    ws_t, ws = da.workspace(nbytes)
    idx, dist = _full((s.N + 2) * k, -77, "int64"), _full((s.N + 2) * k, -77.0, "float64")
    nat.call("dbgsom_kneighbors_manhattan", s.x, da.CODE[s.dtype], s.N, s.d, s.ldx, s.w, s.M, s.ldw, k, slab_rows,
             idx.data_ptr() + 8 * k, dist.data_ptr() + 8 * k, ws, nbytes, da.stream())
    _sync()
    idx, dist = idx.cpu().numpy().reshape(s.N + 2, k), dist.cpu().numpy().reshape(s.N + 2, k)
    assert (idx[[0, -1]] == -77).all() and (dist[[0, -1]] == -77.0).all()
    return dist[1:-1], idx[1:-1]


# ---- 1. device level: search and matrix -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,d,M,xpad,wpad,k", mh.RAW_CASES)
def test_search_and_matrix_bit_for_bit(nat, dtype, N, d, M, xpad, wpad, k):
    if k > M:
        k = M
    X, W = mh.raw_case(dtype, N, d, M)
    D = mh.raw_reference(dtype, N, d, M)
    s = Staged(X, W, xpad, wpad)
    dist, idx = raw_bmu(nat, s, k)
    want_dist, want_idx = mh.l1_select(D, k)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
    got = raw_distances(nat, s, ldo=M + (N % 3))
    assert np.array_equal(got, D)
    assert np.array_equal(got.min(axis=1), dist[:, 0])                         # the search's distance is the smallest entry


def test_many_rows_and_few_rows_kernels_and_any_batch_give_the_same_bits(nat):
    dtype, N, d, M = "f32", 8192 + 17, 5, 3
    X, W = mh.raw_case(dtype, N, d, M)
    s = Staged(X, W, 1, 0)
    for k in (1, 2):
        whole_d, whole_i = raw_bmu(nat, s, k)                                  # 16 rows per workgroup
        for row0, n in ((0, 100), (4001, 333), (N - 5, 5), (17, 1)):           # 4 rows per workgroup, other neighbours
            part_d, part_i = raw_bmu(nat, s, k, n=n, row0=row0)
            assert np.array_equal(part_i, whole_i[row0:row0 + n]) and np.array_equal(part_d, whole_d[row0:row0 + n])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_edge_results(nat, dtype):
    rng = np.random.default_rng(2)
    M, d = 300, 6
    W = rng.normal(size=(M, d))
    W = W.astype(np.float32).astype(np.float64)                                # representable as float32 rows
    W[270] = W[14]
    W[200] = W[14]                                                             # bit-identical prototypes
    X = rng.normal(size=(9, d))
    X[0] = W[7]                                                                # a row equal to a prototype
    X[1] = W[270]                                                              # ... to three of them
    X[2, 3] = np.nan
    X[3, 0] = np.inf
    X[4] = 1.0e308 if dtype == "f64" else 3.0e38                               # finite, far away
    X[5, 5] = -np.inf
    X = X.astype(mh.NP_DTYPE[dtype])
    s = Staged(X, W, 2, 1)
    D = mh.l1_distances(X, W)
    for k in (1, 2):
        dist, idx = raw_bmu(nat, s, k)
        want_dist, want_idx = mh.l1_select(D, k)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
        assert idx[0, 0] == 7 and dist[0, 0] == 0.0
        assert idx[1].tolist() == [14, 200][:k] and (dist[1] == 0.0).all()      # ties: the lower index
        for r in (2, 3, 5):                                                     # NaN / infinity: nothing wins
            assert (idx[r] == -1).all() and np.isinf(dist[r]).all()
    assert np.isfinite(D[4]).all() == (dtype == "f32")                          # float64: the sum overflows to +inf
    got = raw_distances(nat, s)
    assert np.array_equal(got, D, equal_nan=True)
    assert np.isnan(got[2]).all() and np.isinf(got[3]).all()
    dist, idx = raw_kneighbors(nat, s, 5)
    want_dist, want_idx = mh.l1_select(D, 5)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
    assert idx[1].tolist()[:3] == [14, 200, 270]


@pytest.mark.parametrize("ldo_extra,off", [(0, 0), (1, 0), (2, 1), (3, 4), (0, 3)])
def test_matrix_layouts(nat, ldo_extra, off):
    """odd and even ldo, output bases on and off 32 bytes, sentinels around the result"""
    X, W = mh.raw_case("f64", 17, 7, 513)
    s = Staged(X, W, 1, 0)
    got = raw_distances(nat, s, ldo=513 + ldo_extra, off=off)
    assert np.array_equal(got, mh.raw_reference("f64", 17, 7, 513))


# ---- 2. device level: the selection ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_kneighbors_against_the_oracle(nat, k, dtype):
    N, d, M = 301, 5, 41                                                       # M odd: the slab's rows are 42 apart
    X, W = mh.raw_case(dtype, N, d, M)
    D = mh.raw_reference(dtype, N, d, M)
    assert (np.sort(D, axis=1)[:, 1:] == np.sort(D, axis=1)[:, :-1]).any()     # equal distances inside rows
    s = Staged(X, W, 3, 1)
    want_dist, want_idx = mh.l1_select(D, k)
    one_d, one_i = raw_kneighbors(nat, s, k)
    assert np.array_equal(one_i, want_idx) and np.array_equal(one_d, want_dist)
    three_d, three_i = raw_kneighbors(nat, s, k, slab_rows=128)                # three slabs against one
    assert np.array_equal(three_i, one_i) and np.array_equal(three_d, one_d)
    if k <= 2:
        dist, idx = raw_bmu(nat, s, k)
        assert np.array_equal(idx, one_i) and np.array_equal(dist, one_d)


@pytest.mark.parametrize("dtype,N,d,M", [("f64", 17, 7, 513), ("f32", 8192 + 17, 5, 3), ("f32", 15, 3, 256)])
def test_kneighbors_across_prototype_blocks_and_row_kernels(nat, dtype, N, d, M):
    """the slab kernel divides the blocks of 256 prototypes over the grid: M = 513 are three; 8192 + 17 rows take the
    many-rows instantiation"""
    X, W = mh.raw_case(dtype, N, d, M)
    D = mh.raw_reference(dtype, N, d, M)
    s = Staged(X, W, 1, 2)
    k = min(5, M)
    dist, idx = raw_kneighbors(nat, s, k)
    want_dist, want_idx = mh.l1_select(D, k)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)


def test_kneighbors_takes_no_root_and_refuses_k_above_M(nat):
    X = np.zeros((3, 1))
    W = np.array([[16.0], [4.0], [9.0]])                                       # distances 16, 4, 9: perfect squares
    s = Staged(X, W)
    dist, idx = raw_kneighbors(nat, s, 3)
    assert idx.tolist() == [[1, 2, 0]] * 3 and dist.tolist() == [[4.0, 9.0, 16.0]] * 3
    lib = nat.load()
    rc = lib.dbgsom_kneighbors_manhattan(s.x, da.CODE["f64"], 3, 1, 1, s.w, 3, 1, 4, 0, 8, 8, 8, 1 << 20, None)
    assert rc == -1 and b"k <= M" in lib.dbgsom_last_error()


# ---- 3. the context calls ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backend():
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0)
    yield be
    be.release()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_queries_in_chunks_and_from_device_rows(backend, dtype):
    import torch

    be = backend
    N, d, M = 301, 5, 41
    X, W = mh.raw_case(dtype, N, d, M)
    D = mh.raw_reference(dtype, N, d, M)
    before = be.sample_traffic()
    one = (be.bmu_manhattan(W, 2, X), be.distances_manhattan(W, X), be.kneighbors_manhattan(W, 5, X))
    moved = be.sample_traffic()
    assert moved["x_upload_bytes"] - before["x_upload_bytes"] == 3 * X.nbytes
    assert moved["x_download_bytes"] - before["x_download_bytes"] == N * (2 * 16 + M * 8 + 5 * 16)
    want2, want5 = mh.l1_select(D, 2), mh.l1_select(D, 5)
    assert np.array_equal(one[0][0], want2[0]) and np.array_equal(one[0][1], want2[1])
    assert np.array_equal(one[1], D)
    assert np.array_equal(one[2][0], want5[0]) and np.array_equal(one[2][1], want5[1])
    d1, i1 = be.bmu_manhattan(W, 1, X)
    assert d1.shape == (N,) and np.array_equal(i1, want2[1][:, 0]) and np.array_equal(d1, want2[0][:, 0])
    keep = (be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows)
    try:                                                                         # several host chunks against one
        be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows = 64, 50, 16
        many = (be.bmu_manhattan(W, 2, X), be.distances_manhattan(W, X), be.kneighbors_manhattan(W, 5, X))
        xt = torch.from_numpy(np.array(X)).cuda()
        wide = torch.full((N, d + 3), float("nan"), dtype=xt.dtype, device="cuda")
        wide[:, :d] = xt
        for rows in (xt, wide[:, :d]):                                           # device rows, contiguous and strided
            now = be.sample_traffic()
            dev = (be.bmu_manhattan(W, 2, rows), be.distances_manhattan(W, rows), be.kneighbors_manhattan(W, 5, rows))
            assert be.sample_traffic() == now                                    # nothing crossed PCIe
            assert all(t.is_cuda for t in (dev[0][0], dev[0][1], dev[1], dev[2][0], dev[2][1]))
            dev = ((dev[0][0].cpu().numpy(), dev[0][1].cpu().numpy()), dev[1].cpu().numpy(),
                   (dev[2][0].cpu().numpy(), dev[2][1].cpu().numpy()))
            for got in (many, dev):
                assert np.array_equal(got[0][0], one[0][0]) and np.array_equal(got[0][1], one[0][1])
                assert np.array_equal(got[1], one[1])
                assert np.array_equal(got[2][0], one[2][0]) and np.array_equal(got[2][1], one[2][1])
    finally:
        be.masked_chunk_rows, be.distances_chunk_rows, be.kneighbors_slab_rows = keep


def test_context_argument_errors_are_status_codes(backend, nat):
    lib = nat.load()
    be = backend
    X, W = mh.raw_case("f64", 17, 5, 2)
    X, W = np.ascontiguousarray(X), np.ascontiguousarray(W)
    idx, dist = np.full((17, 2), -5, dtype=np.int64), np.full((17, 2), -5.0)
    args = (X.ctypes.data, 1, 17, 5, W.ctypes.data, 2)
    err = lib.dbgsom_last_error
    assert lib.dbgsom_ctx_bmu_query_manhattan(be._ctx, X.ctypes.data, 2, 17, 5, W.ctypes.data, 2, 1, idx.ctypes.data,
                                              dist.ctypes.data) == -1 and b"x_dtype" in err()
    assert lib.dbgsom_ctx_bmu_query_manhattan(be._ctx, *args, 3, idx.ctypes.data, dist.ctypes.data) == -1 and b"k must" in err()
    assert lib.dbgsom_ctx_bmu_query_manhattan(be._ctx, *args, 1, None, dist.ctypes.data) == -1 and b"null" in err()
    assert lib.dbgsom_ctx_kneighbors_query_manhattan(be._ctx, *args, 3, idx.ctypes.data, dist.ctypes.data) == -1 and b"k <= M" in err()
    assert lib.dbgsom_ctx_distances_query_manhattan(be._ctx, *args, None) == -1 and b"null" in err()
    assert lib.dbgsom_ctx_distances_query_manhattan_device(be._ctx, 8, 1, 17, 5, 4, W.ctypes.data, 2, 8, 2) == -1     # ldx < d
    assert lib.dbgsom_ctx_distances_query_manhattan_device(be._ctx, 8, 1, 17, 5, 5, W.ctypes.data, 2, 8, 1) == -1 and b"ldo" in err()
    assert (idx == -5).all() and (dist == -5.0).all()                            # nothing was launched
    assert lib.dbgsom_ctx_bmu_manhattan(be._ctx, W.ctypes.data, 2, 1, idx.ctypes.data, dist.ctypes.data) == -4       # no rows loaded
    Xf = np.ascontiguousarray(X, dtype=np.float32)
    be.load(Xf, storage="bf16")
    try:
        with pytest.raises(ValueError, match="bfloat16"):
            nat.call("dbgsom_ctx_bmu_manhattan", be._ctx, W.ctypes.data, 2, 1, idx.ctypes.data, dist.ctypes.data)
    finally:
        be.release()
    be.load(X)
    try:
        be.set_sample_weight(np.ones(17))
        with pytest.raises(ValueError, match="sample weights"):
            nat.call("dbgsom_ctx_bmu_manhattan", be._ctx, W.ctypes.data, 2, 1, idx.ctypes.data, dist.ctypes.data)
        be.set_sample_weight(None)
        be.set_metric("manhattan")
        d2, i2 = be.bmu(W, 2)                                                     # the resident search
        want = mh.l1_bmu(X, W, 2)
        assert np.array_equal(i2, want[1]) and np.array_equal(d2, want[0])
        out = np.empty((2, 5))                                                    # the epoch before set_topology
        rc = lib.dbgsom_ctx_epoch_manhattan(be._ctx, W.ctypes.data, 2, 0.1, 1.0, 0, out.ctypes.data, dist.ctypes.data,
                                            dist.ctypes.data, dist.ctypes.data, None, None)
        assert rc == -4 and b"topology" in err()
    finally:
        be.release()
    assert be._metric == "euclidean"


# ---- 4. one epoch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["compact", "aligned"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_epoch_against_the_stand_in(backend, dtype, layout):
    N, d, M = 300, 7, 9
    rng = np.random.default_rng(9)
    X = (rng.normal(size=(N, d)) * 1.5).astype(mh.NP_DTYPE[dtype])
    W = np.asarray(X[rng.choice(N, M, replace=False)], dtype=np.float64) + 0.1 * rng.normal(size=(M, d))
    hop = gi.lattice_hops(3, 3)
    sigma, gamma = 1.4, float(np.var(X, axis=0).sum() ** -1)
    ref_be = mh.ManhattanOracleBackend().load(X)
    ref_be.set_metric("manhattan")
    ref = ref_be.epoch_manhattan(W, hop, sigma, gamma, layout, want_assignments=True)
    be = backend.load(X)
    try:
        be.set_metric("manhattan")
        res = be.epoch_manhattan(W, hop, sigma, gamma, layout, want_assignments=True)
        assert np.array_equal(res.winners, ref.winners) and np.array_equal(res.distances, ref.distances)
        np.testing.assert_allclose(res.new_weights, ref.new_weights, rtol=W_RTOL, atol=W_ATOL)
        np.testing.assert_allclose(res.errors, ref.errors, rtol=E_RTOL)
        assert np.array_equal(res.activations, ref.activations)
        assert res.change_total == pytest.approx(ref.change_total, rel=CHG_REL)
        assert be.quantization_error(W) == float(np.mean(ref.distances))              # a host mean of the same bits
        with pytest.raises(ValueError, match="resident"):
            from dbgsom_amd.backend import RESIDENT
            be.epoch_manhattan(RESIDENT, hop, sigma, gamma, layout)
    finally:
        be.release()


def test_the_resident_workspace_belongs_to_the_context(backend, nat):
    """the transposed prototypes and the float64 copy of float32 residents are a buffer of the context like the others:
    counted in "device_bytes" (the list dbgsom_ctx_destroy frees), 10 MB here where every other buffer the call grows
    takes 1 MiB"""
    N, d, M = 20000, 64, 4
    X = np.zeros((N, d), dtype=np.float32)
    W = np.ones((M, d))
    be = backend.load(X)
    try:
        be.set_metric("manhattan")
        before = be._get("device_bytes")
        dist, idx = be.bmu(W, 1)
        assert (idx == 0).all() and (dist == float(d)).all()
        need = nat.load().dbgsom_bmu_manhattan_workspace_bytes(da.CODE["f32"], N, d, M)
        assert need >= N * d * 8 and be._get("device_bytes") - before >= need
    finally:
        be.release()


# ---- 5. the estimators ------------------------------------------------------------------------------------------------
def _fit_pair(cls, backend, **kw):
    X, lab = mh.blobs()
    args = (X, lab) if cls.__name__ == "SomClassifier" else (X,)
    gpu = cls(backend=backend, metric="manhattan", **mh.FIT_KW, **kw).fit(*args)
    cpu = cls(backend=mh.ManhattanOracleBackend(), metric="manhattan", **mh.FIT_KW, **kw).fit(*args)
    return gpu, cpu, X, lab


def test_somvq_on_the_device_against_the_stand_in(backend):
    import torch
    from dbgsom_amd import SomVQ

    X, _ = mh.blobs()
    eu_before = SomVQ(backend=backend, **mh.FIT_KW).fit(X)
    gpu, cpu, X, _ = _fit_pair(SomVQ, backend)
    assert len(gpu.weights_) == len(cpu.weights_) and np.array_equal(gpu.labels_, cpu.labels_)
    np.testing.assert_allclose(gpu.weights_, cpu.weights_, rtol=FIT_RTOL, atol=FIT_ATOL)
    assert gpu.quantization_error_ == pytest.approx(cpu.quantization_error_, rel=FIT_RTOL)
    assert np.array_equal(gpu.predict(X), gpu.labels_)
    D = gpu.prototype_distances(X)
    assert np.array_equal(D, mh.l1_distances(X, gpu.weights_))
    k = min(5, len(gpu.weights_))
    dist, idx = gpu.kneighbors(X, n_neighbors=k)
    assert np.array_equal(idx[:, 0], gpu.predict(X)) and np.array_equal(dist, np.take_along_axis(D, idx, axis=1))
    xt = torch.from_numpy(np.array(X)).cuda()                                     # the same queries from a tensor
    td, ti = gpu.kneighbors(xt, n_neighbors=k)
    assert td.is_cuda and ti.is_cuda and gpu.predict(xt).is_cuda and gpu.prototype_distances(xt).is_cuda
    assert np.array_equal(td.cpu().numpy(), dist) and np.array_equal(ti.cpu().numpy(), idx)
    assert np.array_equal(gpu.predict(xt).cpu().numpy(), gpu.labels_)
    assert np.array_equal(gpu.prototype_distances(xt).cpu().numpy(), D)
    assert gpu.calculate_quantization_error(xt) == gpu.calculate_quantization_error(X)
    bad = xt.clone()
    bad[3, 1] = float("nan")                                                      # a tensor is validated on its device
    for call in (gpu.predict, gpu.prototype_distances, lambda a: gpu.kneighbors(a, 2), gpu.calculate_quantization_error):
        with pytest.raises(ValueError, match="NaN"):
            call(bad)
    nan_ok = SomVQ(backend=backend, metric="manhattan", missing_values="nan", **mh.FIT_KW).fit(X)
    with pytest.raises(ValueError, match="NaN.*missing"):
        nan_ok.predict(bad)
    from_tensor = SomVQ(backend=backend, metric="manhattan", **mh.FIT_KW).fit(xt)
    assert np.array_equal(from_tensor.weights_, gpu.weights_)                     # the fit on rows that live in HBM
    assert np.array_equal(from_tensor.labels_, gpu.labels_)
    eu_after = SomVQ(backend=backend, **mh.FIT_KW).fit(X)
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
    ent_g, ent_c, _, _ = _fit_pair(SomClassifier, backend, growth_criterion="entropy")
    assert len(ent_g.weights_) == len(ent_c.weights_)
    np.testing.assert_allclose(ent_g.weights_, ent_c.weights_, rtol=FIT_RTOL, atol=FIT_ATOL)
