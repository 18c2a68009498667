"""MI355X: the distortion measure -- the energy kernel of csrc/distortion.hip on crafted matrices against its NumPy
restatement bit for bit, the slab driver over the shape table of tests/prototype_distances.py against the restatement
on the exact squared matrix (and against dbgsom_bmu on the same buffers), the context calls (chunks, rows in HBM, CSR,
traffic) and the estimator.  No test asserts on a clock."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import device_abi as da
from tests import distortion as ds
from tests import golden_inputs as gi
from tests import prototype_distances as pd

pytestmark = pytest.mark.gpu

GUARD = 8          # sentinel elements in front of and behind either result


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


def _sync():
    import torch

    torch.cuda.synchronize()


def _full(shape, value, dtype):
    import torch

    return torch.full(shape, value, dtype=getattr(torch, dtype), device="cuda")


def _bits(a):
    """the bit patterns, every NaN as one: which NaN comes out of 0 * inf, or of a sum of two different NaNs, is the
    processor's choice (sign and payload), not IEEE's"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


def _align_up(nbytes, a=256):
    return (nbytes + a - 1) // a * a


def _padded(A, ld, fill=np.nan):
    """the rows of A `ld` elements apart on the device, what lies between them filled with `fill`"""
    host = np.full((A.shape[0], ld), fill)
    host[:, :A.shape[1]] = A
    return da.dev(host)


class _Results:
    """bmu (int64) and e (float64) of N values, each with GUARD sentinel elements on either side"""

    def __init__(self, N):
        self.N = N
        self.bmu = _full((N + 2 * GUARD,), ds.BMU_SENTINEL, "int64")
        self.e = _full((N + 2 * GUARD,), ds.SENTINEL, "float64")
        self.bmu_ptr, self.e_ptr = self.bmu.data_ptr() + 8 * GUARD, self.e.data_ptr() + 8 * GUARD

    def read(self):
        """-> (e, bmu); the sentinels around both must be untouched"""
        bmu, e = self.bmu.cpu().numpy(), self.e.cpu().numpy()
        n = self.N
        assert (np.concatenate([bmu[:GUARD], bmu[GUARD + n:]]) == ds.BMU_SENTINEL).all(), "a write outside bmu"
        assert (_bits(np.concatenate([e[:GUARD], e[GUARD + n:]])) == _bits(np.float64(ds.SENTINEL))).all(), \
            "a write outside e"
        return e[GUARD:GUARD + n].copy(), bmu[GUARD:GUARD + n].copy()


# ---- 1. dbgsom_energy_rows on crafted matrices ----------------------------------------------------------------------
def _energy_rows(nat, R, H, ldr_pad=3, ldh_pad=1):
    """the raw call with ldr = M + ldr_pad (NaN in the tail of every row) and ldh = M + ldh_pad"""
    N, M = R.shape
    rd, hd = _padded(R, M + ldr_pad), _padded(H, M + ldh_pad)
    out = _Results(N)
    nat.call("dbgsom_energy_rows", rd.data_ptr(), N, M, M + ldr_pad, hd.data_ptr(), M + ldh_pad, out.bmu_ptr, out.e_ptr,
             da.stream())
    _sync()
    return out.read()


@pytest.mark.parametrize("case", ds.ROWS_CASES, ids=ds.ROWS_IDS)
def test_energy_rows_against_the_restatement(nat, case):
    N, M = case
    R, H = ds.rows_matrix(case), ds.rows_factors(case)
    e, bmu = _energy_rows(nat, R, H)
    want_b, want_e = ds.energy_rows(R, H)
    assert np.array_equal(bmu, want_b)
    assert np.array_equal(_bits(e), _bits(want_e))
    if N >= ds.ROWS_KINDS:
        assert bmu[0] == 0 and bmu[1] == (63 if M > 63 else 0)        # equal minima at lanes 0 / 63 / 64
        assert bmu[2] == -1 and np.isnan(e[2])                        # a row of all NaN
        assert M == 1 or np.isposinf(e[3])                            # one +inf under h > 0
    dense = _energy_rows(nat, R, H, ldr_pad=0, ldh_pad=0)             # contiguous rows: the same bytes
    assert np.array_equal(dense[1], bmu) and np.array_equal(_bits(dense[0]), _bits(e))


@pytest.mark.parametrize("case", [(5, 65), (300, 129), (4, 257)], ids=["N5-M65", "N300-M129", "N4-M257"])
def test_identity_and_all_ones_factors(nat, case):
    N, M = case
    R = ds.rows_matrix(case)
    e, bmu = _energy_rows(nat, R, np.eye(M))
    want_b, want_e = ds.energy_rows(R, np.eye(M))
    assert np.array_equal(bmu, want_b) and np.array_equal(_bits(e), _bits(want_e))
    clean = np.isfinite(R).all(axis=1)
    assert clean.sum() >= N - ds.ROWS_KINDS + 2
    assert np.array_equal(e[clean], R[clean, bmu[clean]])             # H = I: the winning value itself
    assert bmu[3] >= 0 and np.isnan(e[3])                             # one +inf under h = 0: 0 * inf
    e1, b1 = _energy_rows(nat, R, np.ones((M, M)))
    w1 = ds.energy_rows(R, np.ones((M, M)))
    assert np.array_equal(b1, w1[0]) and np.array_equal(_bits(e1), _bits(w1[1]))
    assert np.isposinf(e1[3])
    np.testing.assert_allclose(e1[clean], R[clean].sum(axis=1), rtol=(-(-M // 64) + 8) * ds.U)


# ---- 2. dbgsom_neighborhood_energy ----------------------------------------------------------------------------------
def _norms(nat, A, ld, off, dtype):
    t, ptr = da.stage(A, ld, off, dtype)
    out = _full((A.shape[0],), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], A.shape[0], A.shape[1], ld, out.data_ptr(), da.stream())
    return out, t, ptr


def _neighborhood_energy(nat, dtype, X, W, H, ldx, x_off, slab_rows=0, with_bmu=False, poison=False, short=0):
    """dbgsom_neighborhood_energy with xx / ww from dbgsom_row_sqnorms on the same buffers and ldh = M + 1 -> (e, bmu),
    and with with_bmu the winners of dbgsom_bmu (k = 1) on the very same buffers.  poison: the workspace holds NaN."""
    import torch

    N, d = X.shape
    M = W.shape[0]
    xx, _xt, xptr = _norms(nat, X, ldx, x_off, dtype)
    ww, _wt, wptr = _norms(nat, W, d, 0, "f64")
    hd = _padded(H, M + 1)
    nbytes = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, slab_rows)
    ws, wsp = da.workspace(nbytes)
    if poison:
        ws.view(torch.float64)[:] = float("nan")
    out = _Results(N)
    nat.call("dbgsom_neighborhood_energy", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(),
             hd.data_ptr(), M + 1, slab_rows, out.bmu_ptr, out.e_ptr, wsp, nbytes - short, da.stream())
    search = None
    if with_bmu:
        idx, dist = _full((N,), -7, "int64"), _full((N,), float("nan"), "float64")
        nat.call("dbgsom_bmu", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), 1, 0,
                 idx.data_ptr(), dist.data_ptr(), da.stream())
        _sync()
        search = idx.cpu().numpy()
    _sync()
    return (out.read(), search) if with_bmu else out.read()


@pytest.mark.parametrize("i", range(len(pd.CASES)), ids=pd.CASE_IDS)
def test_neighborhood_energy_against_the_restatement(nat, i):
    case = pd.CASES[i]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    R, H, want_b, want_e = ds.case_reference(case)
    (e, bmu), search = _neighborhood_energy(nat, dtype, X, W, H, d + pad, x_off, with_bmu=True, poison=True)
    assert np.array_equal(bmu, want_b) and np.array_equal(bmu, search)
    assert np.array_equal(_bits(e), _bits(want_e))


def test_three_slabs_equal_one(nat):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = ds.SLAB_CASE
    X, W, _ = pd.case_data(ds.SLAB_CASE)
    R, H, want_b, want_e = ds.case_reference(ds.SLAB_CASE)
    assert N == 300
    one = _neighborhood_energy(nat, dtype, X, W, H, d + pad, x_off)
    three = _neighborhood_energy(nat, dtype, X, W, H, d + pad, x_off, slab_rows=100, poison=True)
    assert nat.load().dbgsom_kneighbors_workspace_bytes(N, M, 100) == _align_up(100 * (M + M % 2) * 8)
    assert np.array_equal(three[1], one[1]) and np.array_equal(_bits(three[0]), _bits(one[0]))
    assert np.array_equal(one[1], want_b) and np.array_equal(_bits(one[0]), _bits(want_e))


def test_short_workspace_is_enomem(nat):
    from dbgsom_amd._native import DbgsomNativeError

    case = pd.CASES[0]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    nbytes = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, 0)
    with pytest.raises(DbgsomNativeError, match="%d bytes, %d needed" % (nbytes - 1, nbytes)) as err:
        _neighborhood_energy(nat, dtype, X, W, ds.gaussian_factors(M), d + pad, x_off, short=1)
    assert err.value.code == -3
    _sync()


# ---- 3. the context calls -------------------------------------------------------------------------------------------
def test_host_path_in_chunks(nat, be):
    case = pd.CASES[5]                                               # f32, N = 300, M = 33, d = 784
    X, W, _ = pd.case_data(case)
    R, H, want_b, want_e = ds.case_reference(case)
    before = be.sample_traffic()
    e, bmu = be.neighborhood_energy(W, H, X)
    after = be.sample_traffic()
    assert e.dtype == np.float64 and bmu.dtype == np.int64 and e.shape == bmu.shape == (300,)
    assert np.array_equal(bmu, want_b) and np.array_equal(_bits(e), _bits(want_e))
    assert after["x_upload_bytes"] - before["x_upload_bytes"] == X.nbytes + H.nbytes      # the rows and H, once
    assert after["x_upload_calls"] - before["x_upload_calls"] == 2
    assert after["x_download_bytes"] - before["x_download_bytes"] == 300 * 16             # not N x M x 8
    be.distances_chunk_rows, be.kneighbors_slab_rows = 100, 64
    try:
        e3, b3 = be.neighborhood_energy(W, H, X)
        assert be.sample_traffic()["x_upload_calls"] - after["x_upload_calls"] == 3 + 1   # three chunks, H once
    finally:
        be.distances_chunk_rows, be.kneighbors_slab_rows = 0, 0
    assert np.array_equal(b3, bmu) and np.array_equal(_bits(e3), _bits(e))
    X64 = np.ascontiguousarray(X[:, :17], dtype=np.float64)           # d = 17: padded on the way up
    e17, b17 = be.neighborhood_energy(W[:, :17], H, X64)
    w17 = ds.energy_rows(ds.squared_matrix(X64, W[:, :17]), H)
    assert np.array_equal(b17, w17[0]) and np.array_equal(_bits(e17), _bits(w17[1]))
    with pytest.raises(ValueError, match="H must be"):
        be.neighborhood_energy(W, H[:, :5], X)


def test_device_path_equals_host_path(be):
    import torch

    rng = np.random.default_rng(7)
    W48, W17 = rng.normal(size=(37, 48)) * 1.5, rng.normal(size=(37, 17)) * 1.5
    H = ds.gaussian_factors(37)
    X48 = (rng.normal(size=(301, 48)) * 2.0).astype(np.float32)
    X17 = rng.normal(size=(301, 17)) * 2.0
    wide = torch.from_numpy((rng.normal(size=(301, 80)) * 2.0).astype(np.float32)).cuda()
    view = wide[:, 8:56]                                              # strided: ldx = 80 > d, base 32 bytes in
    for W, host, t in ((W48, X48, torch.from_numpy(X48).cuda()),      # borrowed where it lies
                       (W17, X17, torch.from_numpy(X17).cuda()),      # pad-copied on the device
                       (W48, view.cpu().numpy(), view)):
        want_e, want_b = be.neighborhood_energy(W, H, host)
        before = be.sample_traffic()
        e, bmu = be.neighborhood_energy(W, H, t)
        after = be.sample_traffic()
        assert after["x_download_bytes"] == before["x_download_bytes"]                    # no result crossed PCIe
        assert after["x_upload_bytes"] - before["x_upload_bytes"] == H.nbytes             # and of the way up only H
        for got, dtype in ((e, torch.float64), (bmu, torch.int64)):
            assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
            assert tuple(got.shape) == (301,)
        assert np.array_equal(bmu.cpu().numpy(), want_b) and np.array_equal(_bits(e.cpu().numpy()), _bits(want_e))
        w = ds.energy_rows(ds.squared_matrix(np.ascontiguousarray(host), W), H)
        assert np.array_equal(want_b, w[0]) and np.array_equal(_bits(want_e), _bits(w[1]))


def test_csr_equals_dense(be):
    rng = np.random.default_rng(64)
    Xs = sp.random(203, 64, density=0.3, format="csr", dtype=np.float32, random_state=3)
    W = rng.normal(size=(41, 64))
    H = ds.gaussian_factors(41)
    dense_e, dense_b = be.neighborhood_energy(W, H, Xs.toarray())
    be.distances_chunk_rows = 64
    try:
        e, bmu = be.neighborhood_energy(W, H, Xs)
    finally:
        be.distances_chunk_rows = 0
    assert np.array_equal(bmu, dense_b) and np.array_equal(_bits(e), _bits(dense_e))
    w = ds.energy_rows(ds.squared_matrix(Xs.toarray(), W), H)
    assert np.array_equal(bmu, w[0]) and np.array_equal(_bits(e), _bits(w[1]))


# ---- 4. the estimator -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from dbgsom_amd import SomVQ

    X, _ = gi.blobs_f32(1500, 24, 5, n_centers=12)
    est = SomVQ(random_state=0, n_iter=30, max_neurons=60, spreading_factor=0.9).fit(X)
    return est, X


def test_estimator_host_tensor_and_csr(fitted):
    import torch

    est, X = fitted
    X = X[:500]
    M = len(est.weights_)
    assert 20 <= M <= 64                                                                  # a few dozen units
    e, bmu = est.sample_distortion(X)
    assert isinstance(e, np.ndarray) and isinstance(bmu, np.ndarray)
    assert e.shape == bmu.shape == (500,) and e.dtype == np.float64 and bmu.dtype == np.int64
    assert np.array_equal(bmu, est.predict(X))
    value = est.calculate_distortion(X)
    assert value == float(np.sum(e)) / 500

    t = torch.from_numpy(X).cuda()
    be = est._engine()
    before = be.sample_traffic()
    e_t, bmu_t = est.sample_distortion(t)
    assert be.sample_traffic()["x_download_bytes"] == before["x_download_bytes"]          # no download
    for got, dtype in ((e_t, torch.float64), (bmu_t, torch.int64)):
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
    assert np.array_equal(bmu_t.cpu().numpy(), bmu) and np.array_equal(_bits(e_t.cpu().numpy()), _bits(e))
    assert torch.equal(bmu_t, est.predict(t))
    assert est.calculate_distortion(t) == value                                           # the same float

    Xz = np.where(np.abs(X) < 1.0, 0.0, X).astype(np.float32)
    e_s, bmu_s = est.sample_distortion(sp.csr_matrix(Xz))
    e_d, bmu_d = est.sample_distortion(Xz)
    assert np.array_equal(bmu_s, bmu_d) and np.array_equal(_bits(e_s), _bits(e_d))
    assert est.calculate_distortion(sp.csr_matrix(Xz)) == est.calculate_distortion(Xz)

    # against the route through the full matrix: sqrt, then the square, per term -- three more units
    sigma = est._calculate_current_sigma()
    H = np.exp(-(est._distance_matrix ** 2 / (2 * sigma ** 2)))
    D = est.prototype_distances(X)
    assert np.array_equal(bmu, np.argmin(D, axis=1))
    ref = ds.longdouble_energy(D.astype(np.longdouble) ** 2, H, bmu)
    bound = (-(-M // 64) + 11) * ds.U * ref
    err = np.abs(e.astype(np.longdouble) - ref)
    print("largest error / bound against prototype_distances: %.3f" % float(np.max(err / bound)))
    assert (err <= bound).all()

    # a smaller sigma shrinks every h, so no row's e rises
    smaller, b_small = est.sample_distortion(X, sigma=0.5 * sigma)
    assert np.array_equal(b_small, bmu) and (smaller <= e).all()
    assert est.calculate_distortion(X, sigma=0.5 * sigma) <= value
    # the README's example, as written there
    som, emb = est, t
    e, bmu = som.sample_distortion(emb)
    folded = torch.topk(e, 100).indices
    for s in (0.5, 1.0, 2.0):
        assert som.calculate_distortion(emb, sigma=s) > 0.0
    assert folded.shape == (100,) and torch.equal(bmu, som.predict(emb))
    with pytest.raises(ValueError, match="features"):
        est.sample_distortion(t[:, :10])
    with pytest.raises(ValueError, match="sigma"):
        est.sample_distortion(t, sigma=0.0)
