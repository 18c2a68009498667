"""MI355X: prototype_density -- the fold of csrc/density.hip (dbgsom_range_count_cols) on crafted matrices against the
oracle integer for integer, the slab driver (dbgsom_range_counts) over the shape table of tests/prototype_distances.py
against the oracle on the exact squared matrix and against dbgsom_distances on the same buffers, the context calls
(chunks and slabs that do not divide each other, rows in HBM, CSR, traffic) and the estimators.  Every result lies
between sentinels.  No test asserts on a clock."""
import numpy as np
import pytest
import scipy.sparse as sp

from dbgsom_amd.backend import squared_thresholds
from tests import density as dn
from tests import device_abi as da
from tests import distortion as ds
from tests import golden_inputs as gi
from tests import prototype_distances as pd

pytestmark = pytest.mark.gpu

GUARD = 8          # sentinel elements in front of and behind the counts


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


def _padded(A, ld, fill=np.nan):
    """the rows of A `ld` elements apart on the device, what lies between them filled with `fill`"""
    host = np.full((A.shape[0], ld), fill)
    host[:, :A.shape[1]] = A
    return da.dev(host)


class _Counts:
    """M x n int64 counts with GUARD sentinel elements on either side: the state of the fold, or a whole call's result"""

    def __init__(self, M, n, state=None):
        self.n, self.shape = M * n, (M, n)
        self.c = _full((self.n + 2 * GUARD,), dn.SENTINEL, "int64")
        self.ptr = self.c.data_ptr() + 8 * GUARD
        if state is not None:
            self.c[GUARD:GUARD + self.n] = da.dev(np.ascontiguousarray(state, dtype=np.int64).ravel())

    def read(self):
        """-> the counts; the sentinels around them must be untouched"""
        c = self.c.cpu().numpy()
        assert (np.concatenate([c[:GUARD], c[GUARD + self.n:]]) == dn.SENTINEL).all(), "a write outside the counts"
        return c[GUARD:GUARD + self.n].reshape(self.shape).copy()


# ---- 1. dbgsom_range_count_cols on crafted matrices -----------------------------------------------------------------
def _fold(nat, R, thr, state=None, blocks=None, ldr_pad=3):
    """the raw fold with ldr = M + ldr_pad (NaN in the tails) into a state of zeros (or the given one): one call per
    block of rows ((first, last) pairs; default: one block) -> counts"""
    N, M = R.shape
    n = len(thr)
    rd = _padded(R, M + ldr_pad)
    td = da.dev(np.asarray(thr, dtype=np.float64))
    out = _Counts(M, n, np.zeros((M, n)) if state is None else state)
    for a, b in blocks or [(0, N)]:
        nat.call("dbgsom_range_count_cols", rd.data_ptr() + 8 * a * (M + ldr_pad), b - a, M, M + ldr_pad, td.data_ptr(), n,
                 out.ptr, da.stream())
    _sync()
    return out.read()


@pytest.mark.parametrize("case", dn.COLS_CASES, ids=dn.COLS_IDS)
def test_range_count_cols_against_the_oracle(nat, case):
    N, M, n = case
    R, thr = dn.cols_matrix(case)
    want = dn.range_counts_oracle(R, thr)
    got = _fold(nat, R, thr)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if n >= 2:
        assert np.array_equal(got[:, 0], got[:, 1])                     # duplicated thresholds
    if n >= 3:
        assert np.array_equal(got[:, 2], (R == 0.0).sum(axis=0))       # threshold 0: the exact zeros, nothing else
    if M >= 3:
        assert not got[M - 1].any()                                     # a column of NaN
    assert np.array_equal(_fold(nat, R, thr, ldr_pad=0), got)          # contiguous rows: the same counts
    big = np.full((M, n), 2 ** 32 - 1, dtype=np.int64)                 # a state whose low words are full: the carry
    assert np.array_equal(_fold(nat, R, thr, state=big), want + (2 ** 32 - 1))


FOLD_CASES = [c for c in dn.COLS_CASES if c[0] in (257, 1000)] + dn.COLS_LONG[:2]


@pytest.mark.parametrize("case", FOLD_CASES, ids=[dn.COLS_IDS[dn.COLS_CASES.index(c)] for c in FOLD_CASES])
def test_three_uneven_folds_equal_one(nat, case):
    N, M, n = case
    R, thr = dn.cols_matrix(case)
    a, b = N // 7, N // 7 + (N + 1) // 2
    three = _fold(nat, R, thr, blocks=[(0, a), (a, b), (b, N)])
    assert np.array_equal(three, _fold(nat, R, thr)) and np.array_equal(three, dn.range_counts_oracle(R, thr))


def test_thresholds_as_given_nan_inf_and_neighbours(nat):
    rng = np.random.default_rng(3)
    N, M = 300, 70
    R = rng.random((N, M)) * 4.0
    R[rng.random((N, M)) < 0.1] = np.inf
    R[rng.random((N, M)) < 0.1] = np.nan
    v = 1.2345678
    R[5, :] = v
    R[6, :] = np.nextafter(v, np.inf)
    R[7, :] = np.nextafter(v, -np.inf)
    thr = np.array([v, np.nan, np.inf, np.nextafter(v, -np.inf), -1.0, np.nextafter(v, np.inf), 0.0])
    got = _fold(nat, R, thr)
    assert np.array_equal(got, dn.range_counts_oracle(R, thr))
    assert not got[:, 1].any() and not got[:, 4].any()                 # a NaN threshold counts nothing; nothing is below 0
    assert np.array_equal(got[:, 2], (~np.isnan(R)).sum(axis=0))       # +inf as given: everything but NaN
    assert np.array_equal(got[:, 0] - got[:, 3], np.ones(M)) and np.array_equal(got[:, 5] - got[:, 0], np.ones(M))


def test_fold_argument_errors_write_nothing(nat):
    R = np.ones((10, 5))
    rd, td, out = da.dev(R), da.dev(np.ones(2)), _Counts(5, 2)
    with pytest.raises(ValueError, match="MAX_RADII"):
        nat.call("dbgsom_range_count_cols", rd.data_ptr(), 10, 5, 5, td.data_ptr(), 33, out.ptr, da.stream())
    with pytest.raises(ValueError, match="ldr"):
        nat.call("dbgsom_range_count_cols", rd.data_ptr(), 10, 5, 4, td.data_ptr(), 2, out.ptr, da.stream())
    with pytest.raises(ValueError, match="null pointer"):
        nat.call("dbgsom_range_count_cols", rd.data_ptr(), 10, 5, 5, None, 2, out.ptr, da.stream())
    with pytest.raises(ValueError, match="aligned"):
        nat.call("dbgsom_range_count_cols", rd.data_ptr(), 10, 5, 5, td.data_ptr(), 2, out.ptr + 4, da.stream())
    nat.call("dbgsom_range_count_cols", None, 0, 5, 5, None, 2, None, da.stream())      # no rows: no launch
    _sync()
    assert (out.read() == dn.SENTINEL).all()                           # nothing was written


# ---- 2. dbgsom_range_counts -----------------------------------------------------------------------------------------
def _norms(nat, A, ld, off, dtype):
    t, ptr = da.stage(A, ld, off, dtype)
    out = _full((A.shape[0],), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], A.shape[0], A.shape[1], ld, out.data_ptr(), da.stream())
    return out, t, ptr


def _range_counts(nat, dtype, X, W, thr, ldx, x_off, slab_rows=0, poison=True, short=0, others=False):
    """dbgsom_range_counts with xx / ww from dbgsom_row_sqnorms on the same buffers -> counts, and with others the matrix
    of dbgsom_distances on the very same buffers.  poison: the workspace holds NaN."""
    import torch

    N, d = X.shape
    M, n = W.shape[0], len(thr)
    xx, _xt, xptr = _norms(nat, X, ldx, x_off, dtype)
    ww, _wt, wptr = _norms(nat, W, d, 0, "f64")
    td = da.dev(np.asarray(thr, dtype=np.float64))
    nbytes = nat.load().dbgsom_range_counts_workspace_bytes(N, M, slab_rows)
    ws, wsp = da.workspace(nbytes)
    if poison:
        ws.view(torch.uint8)[:] = 0xff
    out = _Counts(M, n)                                                 # (sentinels inside too: the call zeroes them)
    nat.call("dbgsom_range_counts", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), td.data_ptr(), n,
             slab_rows, out.ptr, wsp, nbytes - short, da.stream())
    _sync()
    if not others:
        return out.read()
    D = _full((N, M), float("nan"), "float64")
    nat.call("dbgsom_distances", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), D.data_ptr(), M,
             da.stream())
    _sync()
    return out.read(), D.cpu().numpy()


@pytest.mark.parametrize("i", range(len(pd.CASES)), ids=pd.CASE_IDS)
def test_range_counts_against_the_oracle_and_the_distances(nat, i):
    case = pd.CASES[i]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    for n in dn.case_nr(i):
        radii, thr, want = dn.case_reference(case, n)
        got, D = _range_counts(nat, dtype, X, W, thr, d + pad, x_off, others=True)
        assert np.array_equal(got, want)                               # the oracle on the exact squared matrix
        assert np.array_equal(got, np.stack([np.count_nonzero(D <= r, axis=0) for r in radii], axis=1))


def test_three_slabs_equal_one(nat):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = dn.SLAB_CASE
    X, W, _ = pd.case_data(dn.SLAB_CASE)
    assert N == 300
    for n in (1, 5, 32):
        _, thr, want = dn.case_reference(dn.SLAB_CASE, n)
        one = _range_counts(nat, dtype, X, W, thr, d + pad, x_off, poison=False)
        three = _range_counts(nat, dtype, X, W, thr, d + pad, x_off, slab_rows=100)
        assert np.array_equal(three, one) and np.array_equal(one, want)


def test_short_workspace_is_enomem_and_no_rows_store_zeros(nat):
    from dbgsom_amd._native import DbgsomNativeError

    case = pd.CASES[0]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    thr = dn.case_reference(case, 3)[1]
    nbytes = nat.load().dbgsom_range_counts_workspace_bytes(N, M, 0)
    with pytest.raises(DbgsomNativeError, match="%d bytes, %d needed" % (nbytes - 1, nbytes)) as err:
        _range_counts(nat, dtype, X, W, thr, d + pad, x_off, short=1)
    assert err.value.code == -3
    _sync()
    out = _Counts(7, 3)
    nat.call("dbgsom_range_counts", None, da.CODE["f32"], 0, 4, 4, None, None, 7, None, None, 3, 0, out.ptr, None, 0,
             da.stream())
    _sync()
    assert not out.read().any()


# ---- 3. the context calls -------------------------------------------------------------------------------------------
def test_host_hbm_and_csr_in_chunks_and_slabs_that_do_not_divide(be):
    import torch

    rng = np.random.default_rng(37)
    N, d, M = 300, 48, 37
    W = rng.normal(size=(M, d)) * 1.5
    X = np.where(rng.random((N, d)) < 0.6, 0.0, rng.normal(size=(N, d)) * 2.0).astype(np.float32)
    X[150:160] = X[20:30]                                                # equal rows in different chunks
    W[3] = X[20]                                                         # a prototype that is a row: r at or near 0
    wide = torch.zeros((N, 80), dtype=torch.float32, device="cuda")
    wide[:, 8:56] = torch.from_numpy(X).cuda()
    view = wide[:, 8:56]                                                 # strided: ldx = 80 > d, base 32 bytes in
    R = ds.squared_matrix(X, W)
    D = np.sqrt(R)
    be.distances_chunk_rows, be.kneighbors_slab_rows = 37, 16
    try:
        for n in (1, 3, 8, 32):
            radii = np.quantile(D, rng.random(n))
            radii[0] = 0.0
            radii[n // 2] = D[11, 5]
            thr = squared_thresholds(radii)
            want = dn.range_counts_oracle(R, thr)
            before = be.sample_traffic()
            host = be.range_counts(W, thr, X)
            after = be.sample_traffic()
            assert isinstance(host, np.ndarray) and host.dtype == np.int64 and host.shape == (M, n)
            assert np.array_equal(host, want)
            assert after["x_download_bytes"] - before["x_download_bytes"] == M * n * 8        # once, not per chunk
            assert after["x_upload_bytes"] - before["x_upload_bytes"] == X.nbytes + n * 8     # the rows and the thresholds
            hbm = be.range_counts(W, thr, view)
            moved = be.sample_traffic()
            assert moved["x_download_bytes"] == after["x_download_bytes"]                      # nothing of X or the result
            assert moved["x_upload_bytes"] - after["x_upload_bytes"] == n * 8                  # ... the thresholds alone
            assert isinstance(hbm, torch.Tensor) and hbm.device == view.device and hbm.dtype == torch.int64
            assert tuple(hbm.shape) == (M, n) and np.array_equal(hbm.cpu().numpy(), host)
            assert np.array_equal(be.range_counts(W, thr, sp.csr_matrix(X)), host)
        assert np.array_equal(host[:, 0], (R == 0.0).sum(axis=0))        # radius 0: the pairs whose r is an exact zero
    finally:
        be.distances_chunk_rows, be.kneighbors_slab_rows = 0, 0
    assert np.array_equal(be.range_counts(W, thr, X), want)               # one chunk, one slab
    X64 = np.ascontiguousarray(X[:, :17], dtype=np.float64)               # d = 17: padded on the way up
    assert np.array_equal(be.range_counts(W[:, :17], thr[:3], X64),
                          dn.range_counts_oracle(ds.squared_matrix(X64, W[:, :17]), thr[:3]))
    empty = be.range_counts(W, thr[:3], X[:0])
    assert isinstance(empty, np.ndarray) and empty.shape == (M, 3) and empty.dtype == np.int64 and not empty.any()
    empty = be.range_counts(W, thr[:3], view[:0])
    assert isinstance(empty, torch.Tensor) and tuple(empty.shape) == (M, 3) and not bool(empty.any())
    with pytest.raises(ValueError, match="MAX_RADII"):
        be.range_counts(W, np.ones(33), X)


# ---- 4. the estimators ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from dbgsom_amd import SomClassifier, SomVQ

    X, y = gi.blobs_f32(1500, 24, 5, n_centers=12)
    vq = SomVQ(random_state=0, n_iter=30, max_neurons=60, spreading_factor=0.9).fit(X)
    clf = SomClassifier(random_state=0, n_iter=12, max_neurons=30).fit(X[:600], y[:600])
    return vq, clf, X


@pytest.mark.parametrize("which", ["SomVQ", "SomClassifier"])
def test_estimator_host_tensor_and_csr(fitted, which):
    import torch

    vq, clf, X = fitted
    est = vq if which == "SomVQ" else clf
    X = X[:500]
    M = len(est.weights_)
    t = torch.from_numpy(X).cuda()
    Xz = np.where(np.abs(X) < 1.0, 0.0, X).astype(np.float32)
    be = est._engine()
    D = est.prototype_distances(X)
    radii = np.quantile(D, [0.02, 0.2, 0.5, 0.9, 0.2])
    radii[3] = D[40, M // 2]
    for radius in (None, float(radii[1]), radii, radii[:1]):
        got = est.prototype_density(X, radius)
        rho = np.atleast_1d(est.density_radius_)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64
        assert got.shape == ((M,) if radius is None or np.ndim(radius) == 0 else (M, len(radius)))
        want = np.stack([np.count_nonzero(D <= r, axis=0) for r in rho], axis=1)
        assert np.array_equal(got.reshape(M, -1), want)                 # the invariant, integer for integer
        assert np.array_equal(got.reshape(M, -1), dn.range_counts_oracle(ds.squared_matrix(X, est.weights_),
                                                                         squared_thresholds(rho)))
        before = be.sample_traffic()
        got_t = est.prototype_density(t, radius)
        assert be.sample_traffic()["x_download_bytes"] == before["x_download_bytes"]      # no download
        assert isinstance(got_t, torch.Tensor) and got_t.device == t.device and got_t.dtype == torch.int64
        assert tuple(got_t.shape) == got.shape and np.array_equal(got_t.cpu().numpy(), got)
        assert np.array_equal(est.prototype_density(sp.csr_matrix(Xz), radius), est.prototype_density(Xz, radius))
    if which == "SomVQ":
        assert est.prototype_density(X, 1e9).tolist() == [len(X)] * M
        # the README's example, as written there
        som, emb = est, t
        P = som.prototype_density(emb)
        profile = som.prototype_density(emb, radius=np.linspace(0.5, 4.0, 8))
        ustar = som.u_star_matrix(emb)
        assert tuple(P.shape) == (M,) and tuple(profile.shape) == (M, 8) and isinstance(som.density_radius_, float)
        assert bool((profile[:, 1:] >= profile[:, :-1]).all())
    U, P = est._get_u_matrix(), est.prototype_density(X).astype(np.float64)
    for rows in (X, t, sp.csr_matrix(X)):
        got = est.u_star_matrix(rows)
        assert isinstance(got, np.ndarray) and got.shape == (M,) and got.dtype == np.float64
        assert np.array_equal(got, U * ((P - P.mean()) / (P.mean() - P.max()) + 1.0))
    assert np.array_equal(est.u_star_matrix(t, 1e9), U)                  # max == mean
    with pytest.raises(ValueError, match="features"):
        est.prototype_density(t[:, :10])
    with pytest.raises(ValueError, match="radii are above the 32"):
        est.prototype_density(t, radius=np.arange(33.0))
