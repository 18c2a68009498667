"""MI355X: kneighbors -- the selection kernel of csrc/kneighbors.hip on crafted matrices against NumPy's lexsort, the
raw device calls over the shape table of tests/prototype_distances.py against the oracle's order bit for bit (and
against dbgsom_bmu and dbgsom_distances on the same buffers), rows with holes, the context calls (chunks, rows in HBM,
CSR) and the estimator.  No test asserts on a clock."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import device_abi as da
from tests import golden_inputs as gi
from tests import kneighbors as kn
from tests import prototype_distances as pd
from tests.test_missing_cpu import RTOL, case as masked_case, punch

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


class _Results:
    """idx (int64) and dist (float64) of N x k, each with GUARD sentinel elements on either side"""

    def __init__(self, N, k):
        self.N, self.k = N, k
        self.idx = _full((N * k + 2 * GUARD,), kn.IDX_SENTINEL, "int64")
        self.dist = _full((N * k + 2 * GUARD,), pd.SENTINEL, "float64")
        self.idx_ptr, self.dist_ptr = self.idx.data_ptr() + 8 * GUARD, self.dist.data_ptr() + 8 * GUARD

    def read(self):
        """-> (dist, idx); the sentinels around both must be untouched"""
        idx, dist = self.idx.cpu().numpy(), self.dist.cpu().numpy()
        n = self.N * self.k
        assert (np.concatenate([idx[:GUARD], idx[GUARD + n:]]) == kn.IDX_SENTINEL).all(), "a write outside idx"
        assert (_bits(np.concatenate([dist[:GUARD], dist[GUARD + n:]])) == _bits(np.float64(pd.SENTINEL))).all(), \
            "a write outside dist"
        return dist[GUARD:GUARD + n].reshape(self.N, self.k).copy(), idx[GUARD:GUARD + n].reshape(self.N, self.k).copy()


# ---- 1. dbgsom_topk_rows on crafted matrices -----------------------------------------------------------------------
@pytest.mark.parametrize("case", kn.TOPK_CASES, ids=kn.TOPK_IDS)
def test_topk_rows_against_lexsort(nat, case):
    N, M, k, pad = case
    R = kn.topk_matrix(case)
    ldr = M + pad
    host = np.full((N, ldr), -1.0)          # (what lies between the rows would win every round if it were read)
    host[:, :M] = R
    rd = da.dev(host)
    out = _Results(N, k)
    nat.call("dbgsom_topk_rows", rd.data_ptr(), N, M, ldr, k, out.idx_ptr, out.dist_ptr, da.stream())
    _sync()
    dist, idx = out.read()
    want_dist, want_idx = kn.topk_lexsort(R, k)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(_bits(dist), _bits(want_dist))
    if N > 1 or kn.TOPK_CASES.index(case) % 4 == 0:
        assert np.array_equal(idx[0], np.arange(k)) and (dist[0] == np.sqrt(2.5)).all()      # the row of equal values
    if N > 1:
        assert (idx[2, k // 2:] == -1).all() and np.isinf(dist[2, k // 2:]).all() and (idx[2, :k // 2] >= 0).all()
        assert (idx[3] == -1).all() and np.isinf(dist[3]).all()


# ---- 2. dbgsom_kneighbors ------------------------------------------------------------------------------------------
def _norms(nat, A, ld, off, dtype):
    t, ptr = da.stage(A, ld, off, dtype)
    out = _full((A.shape[0],), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], A.shape[0], A.shape[1], ld, out.data_ptr(), da.stream())
    return out, t, ptr


def _kneighbors(nat, dtype, X, W, ldx, x_off, ks, slab_rows=0, with_bmu=False):
    """dbgsom_kneighbors for every k of `ks` with xx / ww from dbgsom_row_sqnorms on the same buffers -> {k: (dist,
    idx)}, and with with_bmu the (dist, idx) of dbgsom_bmu for k = 2 on the very same buffers"""
    N, d = X.shape
    M = W.shape[0]
    xx, _xt, xptr = _norms(nat, X, ldx, x_off, dtype)
    ww, _wt, wptr = _norms(nat, W, d, 0, "f64")
    nbytes = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, slab_rows)
    _ws, wsp = da.workspace(nbytes)
    outs = {}
    for k in ks:
        outs[k] = _Results(N, k)
        nat.call("dbgsom_kneighbors", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), k, slab_rows,
                 outs[k].idx_ptr, outs[k].dist_ptr, wsp, nbytes, da.stream())
    search = None
    if with_bmu and M >= 2:
        idx, dist = _full((N, 2), -7, "int64"), _full((N, 2), float("nan"), "float64")
        nat.call("dbgsom_bmu", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), 2, 0,
                 idx.data_ptr(), dist.data_ptr(), da.stream())
        _sync()
        search = dist.cpu().numpy(), idx.cpu().numpy()
    _sync()
    got = {k: r.read() for k, r in outs.items()}
    return (got, search) if with_bmu else got


@pytest.mark.parametrize("i", range(len(pd.CASES)), ids=pd.CASE_IDS)
def test_kneighbors_against_the_oracle(nat, i):
    case = pd.CASES[i]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, D = pd.case_data(case)
    got, search = _kneighbors(nat, dtype, X, W, d + pad, x_off, kn.case_ks(i), with_bmu=True)
    for k, (dist, idx) in got.items():
        want = kn.topk_oracle(X, W, k, D)
        assert np.array_equal(idx, want)
        assert np.array_equal(_bits(dist), _bits(np.take_along_axis(D, want, axis=1)))
        if search is not None and k >= 2:                            # dbgsom_bmu with k = 2 on the same buffers
            assert np.array_equal(idx[:, :2], search[1]) and np.array_equal(_bits(dist[:, :2]), _bits(search[0]))


def test_three_slabs_equal_one(nat):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = kn.SLAB_CASE
    X, W, D = pd.case_data(kn.SLAB_CASE)
    assert N == 300
    k = 16
    one = _kneighbors(nat, dtype, X, W, d + pad, x_off, [k])[k]
    three = _kneighbors(nat, dtype, X, W, d + pad, x_off, [k], slab_rows=128)[k]
    assert nat.load().dbgsom_kneighbors_workspace_bytes(N, M, 128) == 128 * (M + M % 2) * 8
    assert np.array_equal(three[1], one[1]) and np.array_equal(_bits(three[0]), _bits(one[0]))
    assert np.array_equal(one[1], kn.topk_oracle(X, W, k, D))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_planted_collapse(nat, dt):
    X = da.stored(kn.COLLAPSE_X, dt)
    dist, idx = _kneighbors(nat, dt, X, kn.COLLAPSE_W, 2, 0, [3])[3]
    assert np.array_equal(idx, [[1, 0, 2]]) and np.array_equal(dist, [[1.0, 1.0, 3.0]])


def test_short_workspace_is_enomem(nat):
    from dbgsom_amd._native import DbgsomNativeError

    case = pd.CASES[0]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    xx, _xt, xptr = _norms(nat, X, d + pad, x_off, dtype)
    ww, _wt, wptr = _norms(nat, W, d, 0, "f64")
    nbytes = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, 0)
    _ws, wsp = da.workspace(nbytes)
    out = _Results(N, 2)
    with pytest.raises(DbgsomNativeError, match="%d bytes, %d needed" % (nbytes - 1, nbytes)) as e:
        nat.call("dbgsom_kneighbors", xptr, da.CODE[dtype], N, d, d + pad, xx.data_ptr(), wptr, M, ww.data_ptr(), 2, 0,
                 out.idx_ptr, out.dist_ptr, wsp, nbytes - 1, da.stream())
    assert e.value.code == -3
    _sync()
    dist, idx = out.read()
    assert (idx == kn.IDX_SENTINEL).all()                            # nothing was launched


# ---- 3. dbgsom_kneighbors_masked -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("frac", pd.MASKED_FRACS)
@pytest.mark.parametrize("N,d,M", pd.MASKED_SHAPES)
def test_masked_kneighbors(nat, N, d, M, frac, dt):
    X, W, D = masked_case(N, d, M, frac, dt)
    code = da.CODE["f32" if X.dtype == np.float32 else "f64"]
    xd, wd = da.dev(np.array(X)), da.dev(np.array(W))
    lib = nat.load()
    full = _full((N, M), float("nan"), "float64")                    # dbgsom_distances_masked on the same buffers
    nb = lib.dbgsom_bmu_masked_workspace_bytes(code, N, d, M)
    _ws0, wsp0 = da.workspace(nb)
    nat.call("dbgsom_distances_masked", xd.data_ptr(), code, N, d, d, wd.data_ptr(), M, d, full.data_ptr(), M, wsp0, nb,
             da.stream())
    outs = {}
    for k, slab in sorted({(min(M, 2), 0), (min(M, 5), 128), (min(M, 32), 0)}):
        nbytes = lib.dbgsom_kneighbors_masked_workspace_bytes(code, N, d, M, slab)
        _ws, wsp = da.workspace(nbytes)
        outs[k, slab] = _Results(N, k)
        nat.call("dbgsom_kneighbors_masked", xd.data_ptr(), code, N, d, d, wd.data_ptr(), M, d, k, slab,
                 outs[k, slab].idx_ptr, outs[k, slab].dist_ptr, wsp, nbytes, da.stream())
    _sync()
    full = full.cpu().numpy()
    order = np.argsort(D, axis=1, kind="stable")
    for (k, slab), r in outs.items():
        dist, idx = r.read()
        assert np.array_equal(idx, order[:, :k])
        np.testing.assert_allclose(dist, np.take_along_axis(D, idx, axis=1), rtol=RTOL, atol=0.0)
        assert np.array_equal(_bits(dist), _bits(np.take_along_axis(full, idx, axis=1)))


# ---- 4. the context calls ------------------------------------------------------------------------------------------
def _raw(nat, case, k):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    return _kneighbors(nat, dtype, X, W, d + pad, x_off, [k])[k]


def test_host_path_in_chunks(nat, be):
    case = pd.CASES[5]                                               # f32, N = 300, M = 33, d = 784
    X, W, D = pd.case_data(case)
    k = 16
    raw_dist, raw_idx = _raw(nat, case, k)
    before = be.sample_traffic()
    dist, idx = be.kneighbors(W, k, X)
    after = be.sample_traffic()
    assert dist.dtype == np.float64 and idx.dtype == np.int64 and dist.shape == idx.shape == (300, k)
    assert np.array_equal(idx, raw_idx) and np.array_equal(_bits(dist), _bits(raw_dist))
    assert after["x_upload_bytes"] - before["x_upload_bytes"] == X.nbytes
    assert after["x_download_bytes"] - before["x_download_bytes"] == 300 * k * 16      # not N x M x 8
    be.distances_chunk_rows, be.kneighbors_slab_rows = 100, 128
    try:
        assert be.kneighbors_slab_rows == 128
        d3, i3 = be.kneighbors(W, k, X)
        assert be.sample_traffic()["x_upload_calls"] - after["x_upload_calls"] == 3
    finally:
        be.distances_chunk_rows, be.kneighbors_slab_rows = 0, 0
    assert np.array_equal(i3, idx) and np.array_equal(_bits(d3), _bits(dist))
    X64 = np.ascontiguousarray(X[:, :17], dtype=np.float64)           # d = 17: padded on the way up
    d17, i17 = be.kneighbors(W[:, :17], 5, X64)
    D17 = pd.pair_distances(X64, W[:, :17])
    assert np.array_equal(i17, kn.topk_oracle(X64, W[:, :17], 5, D17))
    assert np.array_equal(_bits(d17), _bits(np.take_along_axis(D17, i17, axis=1)))
    with pytest.raises(ValueError, match="k"):
        be.kneighbors(W, 34, X)
    with pytest.raises(ValueError, match="MAX_NEIGHBORS"):
        be.kneighbors(np.vstack([W, W]), 33, X)


def test_device_path_equals_host_path(be):
    import torch

    rng = np.random.default_rng(7)
    W48, W17 = rng.normal(size=(37, 48)) * 1.5, rng.normal(size=(37, 17)) * 1.5
    X48 = (rng.normal(size=(301, 48)) * 2.0).astype(np.float32)
    X17 = rng.normal(size=(301, 17)) * 2.0
    wide = torch.from_numpy((rng.normal(size=(301, 80)) * 2.0).astype(np.float32)).cuda()
    view = wide[:, 8:56]                                              # strided: row stride 80, base 32 bytes in
    for W, host, t, k in ((W48, X48, torch.from_numpy(X48).cuda(), 5),     # borrowed where it lies
                          (W17, X17, torch.from_numpy(X17).cuda(), 32),    # pad-copied on the device
                          (W48, view.cpu().numpy(), view, 9)):
        want_dist, want_idx = be.kneighbors(W, k, host)
        before = be.sample_traffic()
        dist, idx = be.kneighbors(W, k, t)
        assert be.sample_traffic() == before                          # neither X nor the results crossed PCIe
        for got, dtype in ((dist, torch.float64), (idx, torch.int64)):
            assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
            assert tuple(got.shape) == (301, k)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(_bits(dist.cpu().numpy()), _bits(want_dist))
        assert np.array_equal(want_idx, kn.topk_oracle(np.ascontiguousarray(host), W, k))


def test_csr_equals_the_raw_call_on_the_dense_rows(nat, be):
    rng = np.random.default_rng(64)
    Xs = sp.random(203, 64, density=0.3, format="csr", dtype=np.float32, random_state=3)
    W = rng.normal(size=(41, 64))
    raw_dist, raw_idx = _kneighbors(nat, "f32", Xs.toarray(), W, 64, 0, [8])[8]
    be.distances_chunk_rows = 64
    try:
        dist, idx = be.kneighbors(W, 8, Xs)
    finally:
        be.distances_chunk_rows = 0
    assert np.array_equal(idx, raw_idx) and np.array_equal(_bits(dist), _bits(raw_dist))
    dense = be.kneighbors(W, 8, Xs.toarray())
    assert np.array_equal(dense[1], raw_idx) and np.array_equal(_bits(dense[0]), _bits(raw_dist))


def test_masked_context_call_in_chunks(be):
    X, W, D = masked_case(257, 17, 5, 0.3, "float32")
    dist, idx = be.kneighbors_masked(W, 4, X)
    assert np.array_equal(idx, np.argsort(D, axis=1, kind="stable")[:, :4])
    np.testing.assert_allclose(dist, np.take_along_axis(D, idx, axis=1), rtol=RTOL, atol=0.0)
    be.distances_chunk_rows = 100
    try:
        d3, i3 = be.kneighbors_masked(W, 4, X)
    finally:
        be.distances_chunk_rows = 0
    assert np.array_equal(i3, idx) and np.array_equal(_bits(d3), _bits(dist))
    d2, i2 = be.bmu_masked(W, 2, X)
    assert np.array_equal(idx[:, :2], i2) and np.array_equal(_bits(dist[:, :2]), _bits(d2))
    assert np.array_equal(_bits(dist), _bits(np.take_along_axis(be.distances_masked(W, X), idx, axis=1)))
    with pytest.raises(ValueError, match="no observed entry"):
        bad = X.copy()
        bad[3] = np.nan
        be.kneighbors_masked(W, 4, bad)


# ---- 5. the estimator ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from dbgsom_amd import SomVQ

    X, _ = gi.case_X("digits_f32")
    est = SomVQ(missing_values="nan", random_state=0, n_iter=8).fit(X)
    return est, X


def test_estimator_host_and_tensor(fitted):
    import torch

    est, X = fitted
    X = X[:500]
    k = min(7, len(est.weights_))
    dist, idx = est.kneighbors(X, k)
    assert isinstance(dist, np.ndarray) and isinstance(idx, np.ndarray)
    assert dist.shape == idx.shape == (len(X), k) and dist.dtype == np.float64 and idx.dtype == np.int64
    D = est.prototype_distances(X)
    assert np.array_equal(_bits(dist), _bits(np.take_along_axis(D, idx, axis=1)))
    assert np.array_equal(idx[:, 0], est.predict(X))
    d2, i2 = (est._host(a) for a in est._get_winning_neurons(X, 2))
    assert np.array_equal(idx[:, :2], i2) and np.array_equal(_bits(dist[:, :2]), _bits(d2))
    assert np.array_equal(idx, kn.topk_oracle(X, est.weights_, k))
    assert np.array_equal(est.kneighbors(X, k, return_distance=False), idx)
    assert est.kneighbors(X)[1].shape == (len(X), 5)

    t = torch.from_numpy(X).cuda()
    be = est._engine()
    before = be.sample_traffic()
    dist_t, idx_t = est.kneighbors(t, k)
    only_t = est.kneighbors(t, k, return_distance=False)
    assert be.sample_traffic()["x_download_bytes"] == before["x_download_bytes"]          # no download
    for got, dtype in ((dist_t, torch.float64), (idx_t, torch.int64), (only_t, torch.int64)):
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
    assert np.array_equal(idx_t.cpu().numpy(), idx) and np.array_equal(_bits(dist_t.cpu().numpy()), _bits(dist))
    assert torch.equal(only_t, idx_t)
    assert torch.equal(idx_t[:, 0], est.predict(t))
    assert torch.equal(dist_t, est.prototype_distances(t).gather(1, idx_t))
    # the README's example, as written there
    som, emb = est, t
    dist5, idx5 = som.kneighbors(emb, n_neighbors=5)
    w = torch.softmax(-dist5 / dist5.mean(), dim=1)
    protos = torch.from_numpy(som.weights_).to(emb.device)
    smooth = (w[:, :, None] * protos[idx5]).sum(dim=1)
    assert smooth.shape == (len(X), X.shape[1]) and torch.equal(idx5[:, 0], som.predict(emb))
    with pytest.raises(ValueError, match="features"):
        est.kneighbors(t[:, :10])
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit"):
        est.kneighbors(t, len(est.weights_) + 1)


def test_estimator_rows_with_holes_and_sparse(fitted):
    est, X = fitted
    k = min(6, len(est.weights_))
    Xn = punch(X[:300], 0.3, 2)
    Xn[::3] = X[:300:3]                                               # every third row complete
    holes = np.isnan(Xn).any(axis=1)
    dist, idx = est.kneighbors(Xn, k)
    for part in (holes, ~holes):
        d_part, i_part = est.kneighbors(Xn[part], k)
        assert np.array_equal(idx[part], i_part) and np.array_equal(_bits(dist[part]), _bits(d_part))
    assert np.array_equal(_bits(dist), _bits(np.take_along_axis(est.prototype_distances(Xn), idx, axis=1)))
    assert np.array_equal(idx[:, 0], est._host(est.predict(Xn)))
    assert np.array_equal(idx[~holes], kn.topk_oracle(Xn[~holes], est.weights_, k))
    np.testing.assert_allclose(dist, np.take_along_axis(pd.pair_distances(Xn, est.weights_), idx, axis=1), rtol=RTOL,
                               atol=0.0)
    Xs = sp.csr_matrix(X[:300])                                       # digits: half of the cells are zero
    ds, is_ = est.kneighbors(Xs, k)
    dd, id_ = est.kneighbors(X[:300], k)
    assert np.array_equal(is_, id_) and np.array_equal(_bits(ds), _bits(dd))
    empty = est.kneighbors(X[:0], k)
    assert empty[0].shape == empty[1].shape == (0, k)
