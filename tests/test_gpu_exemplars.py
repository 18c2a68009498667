"""MI355X: prototype_exemplars -- the fold of csrc/exemplars.hip (dbgsom_topk_cols) on crafted matrices against the
oracle bit for bit, the slab driver (dbgsom_exemplars) over the shape table of tests/prototype_distances.py against the
oracle on the exact squared matrix, against dbgsom_distances and dbgsom_bmu on the same buffers, the context calls
(chunks and slabs that do not divide each other, rows in HBM, CSR, traffic) and the estimator.  Every result lies
between sentinels.  No test asserts on a clock."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import device_abi as da
from tests import distortion as ds
from tests import exemplars as ex
from tests import golden_inputs as gi
from tests import kneighbors as kn
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
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _padded(A, ld, fill=np.nan):
    """the rows of A `ld` elements apart on the device, what lies between them filled with `fill`"""
    host = np.full((A.shape[0], ld), fill)
    host[:, :A.shape[1]] = A
    return da.dev(host)


class _Pairs:
    """M x k values (float64) and rows (int64), each with GUARD sentinel elements on either side: the state of the fold,
    or the result of a whole call"""

    def __init__(self, M, k, state=None):
        self.n, self.shape = M * k, (M, k)
        self.r = _full((self.n + 2 * GUARD,), ex.SENTINEL, "float64")
        self.i = _full((self.n + 2 * GUARD,), ex.IDX_SENTINEL, "int64")
        self.r_ptr, self.i_ptr = self.r.data_ptr() + 8 * GUARD, self.i.data_ptr() + 8 * GUARD
        if state is not None:
            self.r[GUARD:GUARD + self.n] = da.dev(state[0].ravel())
            self.i[GUARD:GUARD + self.n] = da.dev(state[1].ravel())

    def read(self):
        """-> (r, i); the sentinels around both must be untouched"""
        r, i = self.r.cpu().numpy(), self.i.cpu().numpy()
        n = self.n
        assert (np.concatenate([i[:GUARD], i[GUARD + n:]]) == ex.IDX_SENTINEL).all(), "a write outside the rows"
        assert (np.concatenate([r[:GUARD], r[GUARD + n:]]) == ex.SENTINEL).all(), "a write outside the values"
        return r[GUARD:GUARD + n].reshape(self.shape).copy(), i[GUARD:GUARD + n].reshape(self.shape).copy()


def _same(got, want):
    return np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])


# ---- 1. dbgsom_topk_cols on crafted matrices ------------------------------------------------------------------------
def _fold(nat, R, k, owner=None, row0=0, state=None, blocks=None, ldr_pad=3, short=0):
    """the raw fold with ldr = M + ldr_pad (NaN in the tails) and a scratch full of NaN: dbgsom_topk_cols_init (or the
    given state), then one call per block of rows ((first, last) pairs; default: one block) -> (r, i)"""
    import torch

    N, M = R.shape
    rd = _padded(R, M + ldr_pad)
    od = None if owner is None else da.dev(owner)
    out = _Pairs(M, k, state)
    if state is None:
        nat.call("dbgsom_topk_cols_init", out.r_ptr, out.i_ptr, M, k, da.stream())
    for a, b in blocks or [(0, N)]:
        nbytes = nat.load().dbgsom_topk_cols_workspace_bytes(b - a, M, k)
        ws, wsp = da.workspace(nbytes)
        ws.view(torch.uint8)[:] = 0xff                                   # every float64 a NaN, every row -1
        nat.call("dbgsom_topk_cols", rd.data_ptr() + 8 * a * (M + ldr_pad), b - a, M, M + ldr_pad,
                 None if od is None else od.data_ptr() + 8 * a, row0 + a, k, out.r_ptr, out.i_ptr, wsp, nbytes - short,
                 da.stream())
        _sync()
    return out.read()


@pytest.mark.parametrize("case", ex.COLS_CASES, ids=ex.COLS_IDS)
def test_topk_cols_against_the_oracle(nat, case):
    N, M, k, kind = case
    R, owner = ex.cols_matrix(case), ex.cols_owner(case)
    got = _fold(nat, R, k, owner, row0=11)
    want = ex.topk_cols_oracle(R, k, owner, row0=11)
    assert _same(got, want)
    if kind == "none" and M >= ex.COLS_KINDS and N >= 3:
        assert np.array_equal(got[1][0], [11 + t if t < N else -1 for t in range(k)])    # one value: the lowest rows
        assert got[1][1, 0] == 11 and (k == 1 or got[1][1, 1] == 11 + N - 1)            # equal minima: first, then last
        assert (got[1][2] == -1).all() and np.isposinf(got[0][2]).all()                 # a column of NaN
        assert (got[1][3] >= 0).sum() == min(k // 2, N)                                 # fewer than k below +inf
    if kind == "empty-cell":
        assert (got[1][0] == -1).all()
    if kind == "one-unit":
        assert (got[1][:M - 1] == -1).all()
    dense = _fold(nat, R, k, owner, row0=11, ldr_pad=0)                  # contiguous rows: the same bytes
    assert _same(dense, got)


FOLD_CASES = [c for c in ex.COLS_CASES if c[0] in (257, 1000, 5000)][::3] + [ex.COLS_LONG[1], ex.COLS_LONG[4]]


@pytest.mark.parametrize("case", FOLD_CASES, ids=[ex.COLS_IDS[ex.COLS_CASES.index(c)] for c in FOLD_CASES])
def test_three_uneven_folds_equal_one(nat, case):
    N, M, k, kind = case
    R, owner = ex.cols_matrix(case), ex.cols_owner(case)
    a, b = N // 7, N // 7 + (N + 1) // 2
    three = _fold(nat, R, k, owner, row0=5, blocks=[(0, a), (a, b), (b, N)])
    assert _same(three, _fold(nat, R, k, owner, row0=5))
    assert _same(three, ex.topk_cols_oracle(R, k, owner, row0=5))


@pytest.mark.parametrize("k", [1, 3, 32])
def test_a_state_that_holds_smaller_pairs_stays(nat, k):
    N, M = 300, 65
    rng = np.random.default_rng(k)
    R = rng.random((N, M)) + 1.0
    state = (np.sort(rng.random((M, k)), axis=1), np.arange(M * k, dtype=np.int64).reshape(M, k) + 1000)
    state[0][:, k // 2:] = state[0][:, k // 2][:, None]                   # equal r in the state: rows ascending
    got = _fold(nat, R, k, row0=0, state=state)
    assert _same(got, state)
    assert _same(got, ex.topk_cols_oracle(R, k, state=state))
    half = (np.where(np.arange(k) < (k + 1) // 2, state[0], np.inf), np.where(np.arange(k) < (k + 1) // 2, state[1], -1))
    got = _fold(nat, R, k, row0=0, state=half)                             # a state with empty slots: the new rows fill them
    assert _same(got, ex.topk_cols_oracle(R, k, state=half)) and (got[1] >= 0).all()


def test_rows_near_the_end_of_int32(nat):
    N, M, k, row0 = 300, 70, 9, 2_000_000_000
    case = (N, M, k, "random")
    R, owner = ex.cols_matrix(case), ex.cols_owner(case)
    for own in (None, owner):
        got = _fold(nat, R, k, own, row0=row0, blocks=[(0, 130), (130, 300)])
        assert _same(got, ex.topk_cols_oracle(R, k, own, row0=row0))
        assert got[1].max() >= row0 and got[1][got[1] >= 0].min() >= row0
    top = 2 ** 31 - 1 - N                                                 # the last row is 2^31 - 2
    assert _same(_fold(nat, R, k, None, row0=top), ex.topk_cols_oracle(R, k, None, row0=top))


def test_fold_argument_errors_and_short_workspace(nat):
    from dbgsom_amd._native import DbgsomNativeError

    R = np.ones((10, 5))
    nbytes = nat.load().dbgsom_topk_cols_workspace_bytes(10, 5, 2)
    with pytest.raises(DbgsomNativeError, match="%d bytes, %d needed" % (nbytes - 1, nbytes)) as err:
        _fold(nat, R, 2, short=1)
    assert err.value.code == -3
    with pytest.raises(ValueError, match="MAX_NEIGHBORS"):
        _fold(nat, R, 33)
    with pytest.raises(ValueError, match="row0 \\+ N"):
        _fold(nat, R, 2, row0=2 ** 31 - 10)
    rd, out = da.dev(R), _Pairs(5, 2)
    ws, wsp = da.workspace(nbytes)
    with pytest.raises(ValueError, match="ldr"):
        nat.call("dbgsom_topk_cols", rd.data_ptr(), 10, 5, 4, None, 0, 2, out.r_ptr, out.i_ptr, wsp, nbytes, da.stream())
    with pytest.raises(ValueError, match="null pointer"):
        nat.call("dbgsom_topk_cols", rd.data_ptr(), 10, 5, 5, None, 0, 2, None, out.i_ptr, wsp, nbytes, da.stream())
    with pytest.raises(ValueError, match="16-byte aligned"):
        nat.call("dbgsom_topk_cols", rd.data_ptr(), 10, 5, 5, None, 0, 2, out.r_ptr, out.i_ptr, wsp + 8, nbytes, da.stream())
    _sync()
    out.read()                                                           # nothing was written


# ---- 2. dbgsom_exemplars --------------------------------------------------------------------------------------------
def _norms(nat, A, ld, off, dtype):
    t, ptr = da.stage(A, ld, off, dtype)
    out = _full((A.shape[0],), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], A.shape[0], A.shape[1], ld, out.data_ptr(), da.stream())
    return out, t, ptr


def _exemplars(nat, dtype, X, W, k, ldx, x_off, own_cell=False, slab_rows=0, poison=True, short=0, others=False):
    """dbgsom_exemplars with xx / ww from dbgsom_row_sqnorms on the same buffers -> (dist, idx), and with others the
    matrix of dbgsom_distances and the winners of dbgsom_bmu (k = 1) on the very same buffers.  poison: the workspace
    holds NaN."""
    import torch

    N, d = X.shape
    M = W.shape[0]
    xx, _xt, xptr = _norms(nat, X, ldx, x_off, dtype)
    ww, _wt, wptr = _norms(nat, W, d, 0, "f64")
    nbytes = nat.load().dbgsom_exemplars_workspace_bytes(N, M, k, slab_rows)
    ws, wsp = da.workspace(nbytes)
    if poison:
        ws.view(torch.uint8)[:] = 0xff
    out = _Pairs(M, k)
    nat.call("dbgsom_exemplars", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), k,
             int(own_cell), slab_rows, out.i_ptr, out.r_ptr, wsp, nbytes - short, da.stream())
    _sync()
    if not others:
        return out.read()
    D = _full((N, M), float("nan"), "float64")
    idx, dist = _full((N,), -7, "int64"), _full((N,), float("nan"), "float64")
    nat.call("dbgsom_distances", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), D.data_ptr(), M,
             da.stream())
    nat.call("dbgsom_bmu", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), 1, 0, idx.data_ptr(),
             dist.data_ptr(), da.stream())
    _sync()
    return out.read(), D.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("i", range(len(pd.CASES)), ids=pd.CASE_IDS)
def test_exemplars_against_the_oracle(nat, i):
    case = pd.CASES[i]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    jj = np.arange(M)[:, None]
    for t, k in enumerate(kn.case_ks(i)):
        got, D, search = _exemplars(nat, dtype, X, W, k, d + pad, x_off, others=True)
        assert _same(got, ex.case_reference(case, k))
        filled = got[1] >= 0
        assert np.array_equal(filled.sum(axis=1), np.full(M, min(k, N)))
        assert np.array_equal(_bits(got[0][filled]), _bits(D[got[1][filled], np.broadcast_to(jj, got[1].shape)[filled]]))
        own = _exemplars(nat, dtype, X, W, k, d + pad, x_off, own_cell=True)
        assert _same(own, ex.case_reference(case, k, True))
        filled = own[1] >= 0
        assert np.array_equal(search[own[1][filled]], np.broadcast_to(jj, own[1].shape)[filled])   # dbgsom_bmu's units
        assert np.array_equal(filled.sum(axis=1), np.minimum(k, np.bincount(search, minlength=M)))


def test_three_slabs_equal_one(nat):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = ex.SLAB_CASE
    X, W, _ = pd.case_data(ex.SLAB_CASE)
    assert N == 300
    for k, own in ((1, False), (5, True), (32, False)):
        one = _exemplars(nat, dtype, X, W, k, d + pad, x_off, own_cell=own, poison=False)
        three = _exemplars(nat, dtype, X, W, k, d + pad, x_off, own_cell=own, slab_rows=100)
        assert _same(three, one) and _same(one, ex.case_reference(ex.SLAB_CASE, k, own))


def test_duplicated_rows_tie_by_row(nat):
    case = pd.CASES[7]                                                   # f64, N = 300, M = 31, d = 48
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    X2 = np.ascontiguousarray(np.repeat(X[:40], 2, axis=0))              # rows 2 t and 2 t + 1 are the same row
    R = ds.squared_matrix(X2, W)
    for k, own in ((2, False), (7, False), (8, True)):
        got = _exemplars(nat, dtype, X2, W, k, d + pad, x_off, own_cell=own, slab_rows=7 if own else 0)
        assert _same(got, ex.exemplars_oracle(R, k, own))
        pairs = got[1][:, :k // 2 * 2].reshape(M, -1, 2)
        if not own:
            assert (pairs[:, :, 0] % 2 == 0).all() and (pairs[:, :, 1] == pairs[:, :, 0] + 1).all()


def test_short_workspace_is_enomem(nat):
    from dbgsom_amd._native import DbgsomNativeError

    case = pd.CASES[0]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    nbytes = nat.load().dbgsom_exemplars_workspace_bytes(N, M, 4, 0)
    with pytest.raises(DbgsomNativeError, match="%d bytes, %d needed" % (nbytes - 1, nbytes)) as err:
        _exemplars(nat, dtype, X, W, 4, d + pad, x_off, short=1)
    assert err.value.code == -3
    _sync()


def test_no_rows_store_empty_slots(nat):
    M, k = 7, 3
    nbytes = nat.load().dbgsom_exemplars_workspace_bytes(0, M, k, 0)
    assert nbytes == 2 * 256                                             # the state alone
    ws, wsp = da.workspace(nbytes)
    out = _Pairs(M, k)
    nat.call("dbgsom_exemplars", None, da.CODE["f32"], 0, 4, 4, None, None, M, None, k, 1, 0, out.i_ptr, out.r_ptr, wsp,
             nbytes, da.stream())
    _sync()
    dist, idx = out.read()
    assert np.isposinf(dist).all() and (idx == -1).all()


# ---- 3. the context calls -------------------------------------------------------------------------------------------
def test_host_hbm_and_csr_in_chunks_and_slabs_that_do_not_divide(be):
    import torch

    rng = np.random.default_rng(37)
    N, d, M = 300, 48, 37
    W = rng.normal(size=(M, d)) * 1.5
    X = np.where(rng.random((N, d)) < 0.6, 0.0, rng.normal(size=(N, d)) * 2.0).astype(np.float32)
    X[150:160] = X[20:30]                                                # equal rows in different chunks
    wide = torch.zeros((N, 80), dtype=torch.float32, device="cuda")
    wide[:, 8:56] = torch.from_numpy(X).cuda()
    view = wide[:, 8:56]                                                 # strided: ldx = 80 > d, base 32 bytes in
    R = ds.squared_matrix(X, W)
    be.distances_chunk_rows, be.kneighbors_slab_rows = 37, 16
    try:
        for k, own in ((1, False), (6, True), (32, False), (32, True)):
            want = ex.exemplars_oracle(R, k, own)
            before = be.sample_traffic()
            host = be.exemplars(W, k, X, own_cell=own)
            after = be.sample_traffic()
            assert host[0].dtype == np.float64 and host[1].dtype == np.int64 and host[0].shape == host[1].shape == (M, k)
            assert _same(host, want)
            assert after["x_download_bytes"] - before["x_download_bytes"] == M * k * 16     # once, not per chunk
            assert after["x_upload_bytes"] - before["x_upload_bytes"] == X.nbytes
            assert after["x_upload_calls"] - before["x_upload_calls"] == -(-N // 37)        # nine chunks
            dist, idx = be.exemplars(W, k, view, own_cell=own)
            hbm = be.sample_traffic()
            assert hbm["x_download_bytes"] == after["x_download_bytes"]                      # nothing crossed PCIe
            assert hbm["x_upload_bytes"] == after["x_upload_bytes"]
            for got, dtype in ((dist, torch.float64), (idx, torch.int64)):
                assert isinstance(got, torch.Tensor) and got.device == view.device and got.dtype == dtype
                assert tuple(got.shape) == (M, k)
            assert _same((dist.cpu().numpy(), idx.cpu().numpy()), host)
            assert _same(be.exemplars(W, k, sp.csr_matrix(X), own_cell=own), host)
    finally:
        be.distances_chunk_rows, be.kneighbors_slab_rows = 0, 0
    assert _same(be.exemplars(W, 6, X, own_cell=True), ex.exemplars_oracle(R, 6, True))      # one chunk, one slab
    X64 = np.ascontiguousarray(X[:, :17], dtype=np.float64)              # d = 17: padded on the way up
    assert _same(be.exemplars(W[:, :17], 3, X64), ex.exemplars_oracle(ds.squared_matrix(X64, W[:, :17]), 3))
    empty = be.exemplars(W, 3, X[:0])
    assert np.isposinf(empty[0]).all() and (empty[1] == -1).all() and empty[0].shape == (M, 3)
    dist, idx = be.exemplars(W, 3, view[:0])
    assert isinstance(dist, torch.Tensor) and bool(torch.isinf(dist).all()) and bool((idx == -1).all())
    with pytest.raises(ValueError, match="MAX_NEIGHBORS"):
        be.exemplars(W, 33, X)


# ---- 4. the estimator -----------------------------------------------------------------------------------------------
def _invariants(est, X, k, dist, idx, own_cell):
    """the invariants of the interface on host rows X, dist / idx as NumPy arrays"""
    M = len(est.weights_)
    assert dist.shape == idx.shape == (M, k) and dist.dtype == np.float64 and idx.dtype == np.int64
    D = est.prototype_distances(X)
    filled = idx >= 0
    jj = np.broadcast_to(np.arange(M)[:, None], idx.shape)
    assert np.array_equal(_bits(dist[filled]), _bits(D[idx[filled], jj[filled]]))
    assert np.isposinf(dist[~filled]).all()
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
    want = ex.exemplars_oracle(ds.squared_matrix(X, est.weights_), k, own_cell)
    assert _same((dist, idx), want)


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
    for k, own in ((1, False), (5, True), (8, False)):
        dist, idx = est.prototype_exemplars(X, n_exemplars=k, own_cell=own)
        assert isinstance(dist, np.ndarray) and isinstance(idx, np.ndarray)
        _invariants(est, X, k, dist, idx, own)
        assert np.array_equal(est.prototype_exemplars(X, k, own, return_distance=False), idx)
        before = be.sample_traffic()
        dist_t, idx_t = est.prototype_exemplars(t, n_exemplars=k, own_cell=own)
        assert be.sample_traffic()["x_download_bytes"] == before["x_download_bytes"]      # no download
        for got, dtype in ((dist_t, torch.float64), (idx_t, torch.int64)):
            assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
        assert _same((dist_t.cpu().numpy(), idx_t.cpu().numpy()), (dist, idx))
        only = est.prototype_exemplars(t, k, own, return_distance=False)
        assert isinstance(only, torch.Tensor) and torch.equal(only, idx_t)
        assert _same(est.prototype_exemplars(sp.csr_matrix(Xz), k, own), est.prototype_exemplars(Xz, k, own))
    if which == "SomVQ":
        dist, idx = est.prototype_exemplars(X, 4, own_cell=True)
        filled = idx >= 0
        assert np.array_equal(est.predict(X)[idx[filled]], np.broadcast_to(np.arange(M)[:, None], idx.shape)[filled])
        # the README's example, as written there
        som, emb = est, t
        dist, idx = som.prototype_exemplars(emb, n_exemplars=5)
        medoids = idx[:, 0]
        cell = som.prototype_exemplars(emb, n_exemplars=5, own_cell=True, return_distance=False)
        assert medoids.shape == (M,) and bool((medoids >= 0).all()) and tuple(cell.shape) == (M, 5)
        assert torch.equal(som.predict(emb[cell[cell >= 0]]), torch.nonzero(cell >= 0)[:, 0])
    with pytest.raises(ValueError, match="features"):
        est.prototype_exemplars(t[:, :10])
    with pytest.raises(ValueError, match="n_exemplars"):
        est.prototype_exemplars(t, n_exemplars=33)
