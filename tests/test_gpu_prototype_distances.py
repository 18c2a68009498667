"""MI355X: prototype_distances -- the raw device calls of csrc/distances.hip on small shapes (every launcher form,
strided and unaligned rows, both store widths), the context calls (chunks, rows in HBM, CSR, rows with holes) and
the estimator, against the oracle matrix of tests/prototype_distances.py bit for bit; rows with holes within the
derived RTOL of tests/test_missing_cpu.py.  No test asserts on a clock."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import device_abi as da
from tests import golden_inputs as gi
from tests import prototype_distances as pd
from tests.test_missing_cpu import RTOL, case as masked_case, punch

pytestmark = pytest.mark.gpu

GUARD = 2          # rows of sentinel behind row N - 1


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


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


def _norms(nat, A, ld, off, dtype):
    t, ptr = da.stage(A, ld, off, dtype)
    out = _full((A.shape[0],), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], A.shape[0], A.shape[1], ld, out.data_ptr(), da.stream())
    return out, t, ptr


def _out_buffer(N, ldo, out_off):
    buf = _full((out_off + (N + GUARD) * ldo,), pd.SENTINEL, "float64")
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + 8 * out_off


def _read_out(buf, N, M, ldo, out_off):
    """-> the N x M result; everything else of the buffer must still hold the sentinel, bit for bit"""
    host = buf.cpu().numpy()
    body = host[out_off:].reshape(N + GUARD, ldo)
    untouched = np.concatenate([host[:out_off], body[:N, M:].reshape(-1), body[N:].reshape(-1)])
    assert (_bits(untouched) == _bits(np.float64(pd.SENTINEL))).all(), "a write outside the N x M result"
    return body[:N, :M].copy()


def _distances(nat, dtype, X, W, ldx, x_off, ldo, out_off, with_bmu=False):
    """dbgsom_distances with xx / ww from dbgsom_row_sqnorms on the same buffers (W contiguous) -> D, and with
    with_bmu the (dist, idx) of dbgsom_bmu for k = 1 and k = 2 on the very same buffers"""
    N, d = X.shape
    M = W.shape[0]
    xx, _xt, xptr = _norms(nat, X, ldx, x_off, dtype)
    ww, _wt, wptr = _norms(nat, W, d, 0, "f64")
    buf, optr = _out_buffer(N, ldo, out_off)
    nat.call("dbgsom_distances", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), optr, ldo,
             da.stream())
    searches = []
    for k in ((1, 2) if with_bmu else ()):
        if M < k:
            continue
        idx, dist = _full((N, k), -7, "int64"), _full((N, k), float("nan"), "float64")
        nat.call("dbgsom_bmu", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), k, 0,
                 idx.data_ptr(), dist.data_ptr(), da.stream())
        searches.append((dist, idx))
    _sync()
    D = _read_out(buf, N, M, ldo, out_off)
    return (D, [(a.cpu().numpy(), b.cpu().numpy()) for a, b in searches]) if with_bmu else D


# ---- 1. dbgsom_distances -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pd.CASES, ids=pd.CASE_IDS)
def test_distances_against_the_oracle(nat, case):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, want = pd.case_data(case)
    D, searches = _distances(nat, dtype, X, W, d + pad, x_off, M + ldo_pad, out_off, with_bmu=True)
    assert np.array_equal(D, want)
    if M >= 3:
        assert np.array_equal(_bits(D[:, 0]), _bits(D[:, -1]))       # the duplicated prototype: identical columns
        assert D[N // 2, M // 2] == 0.0                              # the row that is a prototype
    rows = np.arange(N)
    for dist, idx in searches:                                       # dbgsom_bmu on the same buffers
        assert np.array_equal(np.take_along_axis(D, idx, axis=1), dist)
        assert np.array_equal(D.min(axis=1), dist[:, 0])
        # (the oracle has no two r under one square root at the minimum of these inputs:
        #  tests/test_prototype_distances_cpu.py)
        assert np.array_equal(D.argmin(axis=1), idx[:, 0])
    assert np.array_equal(D[rows, want.argmin(axis=1)], want.min(axis=1))


@pytest.mark.parametrize("case", [pd.CASES[2], pd.CASES[9], pd.CASES[15], pd.CASES[23]],
                         ids=[pd.CASE_IDS[i] for i in (2, 9, 15, 23)])
def test_permuted_prototypes_and_split_rows(nat, case):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, want = pd.case_data(case)
    perm = np.random.default_rng(M).permutation(M)
    D = _distances(nat, dtype, X, np.ascontiguousarray(W[perm]), d + pad, x_off, M + ldo_pad, out_off)
    assert np.array_equal(_bits(D), _bits(want[:, perm]))
    h = N // 2 + 1                                                    # halves that are no multiple of a tile
    top = _distances(nat, dtype, np.ascontiguousarray(X[:h]), W, d + pad, x_off, M + ldo_pad, out_off)
    bottom = _distances(nat, dtype, np.ascontiguousarray(X[h:]), W, d + pad, x_off, M + ldo_pad, out_off)
    assert np.array_equal(_bits(np.vstack([top, bottom])), _bits(want))


def test_nan_row_gives_nan_row(nat):
    case = pd.CASES[1]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, want = pd.case_data(case)
    X = X.copy()
    X[5, 7] = np.nan
    D = _distances(nat, dtype, X, W, d + pad, x_off, M + ldo_pad, out_off)
    assert np.isnan(D[5]).all()
    keep = np.arange(N) != 5
    assert np.array_equal(D[keep], want[keep])


# ---- 2. dbgsom_distances_masked ------------------------------------------------------------------------------------
def _masked(nat, X, W, ldo_pad=3, with_bmu=False):
    import torch

    N, d = X.shape
    M = W.shape[0]
    dt = "f32" if X.dtype == np.float32 else "f64"
    xd, wd = da.dev(np.array(X)), da.dev(np.array(W))
    nbytes = nat.load().dbgsom_bmu_masked_workspace_bytes(da.CODE[dt], N, d, M)
    _ws, wsp = da.workspace(nbytes)
    ldo = M + ldo_pad
    buf, optr = _out_buffer(N, ldo, 1)
    nat.call("dbgsom_distances_masked", xd.data_ptr(), da.CODE[dt], N, d, d, wd.data_ptr(), M, d, optr, ldo, wsp, nbytes,
             da.stream())
    found = None
    if with_bmu:
        idx, dist = _full((N, 2), -7, "int64"), _full((N, 2), float("nan"), "float64")
        _ws2, wsp2 = da.workspace(nbytes)
        nat.call("dbgsom_bmu_masked", xd.data_ptr(), da.CODE[dt], N, d, d, wd.data_ptr(), M, d, 2, idx.data_ptr(),
                 dist.data_ptr(), wsp2, nbytes, da.stream())
        torch.cuda.synchronize()
        found = dist.cpu().numpy(), idx.cpu().numpy()
    _sync()
    D = _read_out(buf, N, M, ldo, 1)
    return (D, found) if with_bmu else D


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("frac", pd.MASKED_FRACS)
@pytest.mark.parametrize("N,d,M", pd.MASKED_SHAPES)
def test_masked_distances(nat, N, d, M, frac, dt):
    X, W, want = masked_case(N, d, M, frac, dt)
    D, (dist, idx) = _masked(nat, X, W, with_bmu=True)
    np.testing.assert_allclose(D, want, rtol=RTOL, atol=0.0)
    assert np.array_equal(np.take_along_axis(D, idx, axis=1), dist)  # dbgsom_bmu_masked's distances, bit for bit
    assert np.array_equal(D.min(axis=1), dist[:, 0])


def test_masked_row_equal_to_a_prototype_and_row_without_entries(nat):
    X, W, _ = masked_case(257, 17, 5, 0.3, "float64")
    X, W = X.copy(), W.copy()
    obs = ~np.isnan(X[11])
    W[3, obs] = X[11, obs]                # equal on the observed entries, different elsewhere
    X[20] = np.nan                        # no observed entry: NaN at the device level
    D = _masked(nat, X, W)
    assert D[11, 3] == 0.0 and (D[11, [0, 1, 2, 4]] > 0).all()
    assert np.isnan(D[20]).all() and not np.isnan(np.delete(D, 20, axis=0)).any()


# ---- 3. the context calls ------------------------------------------------------------------------------------------
def test_host_path_in_chunks(be):
    X, W, want = pd.case_data(("f32", 300, 100, 784, 0, 0, 0, 1))
    before = be.sample_traffic()
    assert be.distances_chunk_rows == 0
    one = be.distances(W, X)
    after = be.sample_traffic()
    assert np.array_equal(one, want)
    assert after["x_upload_bytes"] - before["x_upload_bytes"] == X.nbytes
    assert after["x_download_bytes"] - before["x_download_bytes"] == one.nbytes
    be.distances_chunk_rows = 100
    try:
        assert be.distances_chunk_rows == 100
        three = be.distances(W, X)
        assert be.sample_traffic()["x_upload_calls"] - after["x_upload_calls"] == 3
    finally:
        be.distances_chunk_rows = 0
    assert np.array_equal(_bits(three), _bits(one))
    X64 = np.ascontiguousarray(X[:, :17], dtype=np.float64)           # d = 17: padded on the way up
    assert np.array_equal(be.distances(W[:, :17], X64), pd.pair_distances(X64, W[:, :17]))


def test_device_path_equals_host_path(be):
    import torch

    rng = np.random.default_rng(7)
    W48, W17 = rng.normal(size=(37, 48)) * 1.5, rng.normal(size=(37, 17)) * 1.5
    X48 = (rng.normal(size=(301, 48)) * 2.0).astype(np.float32)
    X17 = rng.normal(size=(301, 17)) * 2.0
    wide = torch.from_numpy((rng.normal(size=(301, 80)) * 2.0).astype(np.float32)).cuda()
    view = wide[:, 8:56]                                              # strided: row stride 80, base 32 bytes in
    for W, host, t in ((W48, X48, torch.from_numpy(X48).cuda()),      # borrowed where it lies
                       (W17, X17, torch.from_numpy(X17).cuda()),      # pad-copied on the device
                       (W48, view.cpu().numpy(), view)):
        want = be.distances(W, host)
        before = be.sample_traffic()
        got = be.distances(W, t)
        assert be.sample_traffic() == before                          # neither X nor the result crossed PCIe
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == torch.float64
        assert tuple(got.shape) == want.shape
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
        assert np.array_equal(want, pd.pair_distances(np.ascontiguousarray(host), W))


@pytest.mark.parametrize("d,density", [(64, 0.3), (1100, 0.04)])
def test_csr_equals_dense(be, d, density):
    rng = np.random.default_rng(d)
    Xs = sp.random(203, d, density=density, format="csr", dtype=np.float32, random_state=3)
    W = rng.normal(size=(41, d))
    dense = be.distances(W, Xs.toarray())
    be.distances_chunk_rows = 64
    try:
        got = be.distances(W, Xs)
    finally:
        be.distances_chunk_rows = 0
    assert np.array_equal(_bits(got), _bits(dense))
    assert np.array_equal(_bits(be.distances(W, Xs.astype(np.float64))), _bits(be.distances(W, Xs.toarray().astype(np.float64))))


def test_masked_context_call_in_chunks(be):
    X, W, want = masked_case(257, 17, 5, 0.3, "float32")
    one = be.distances_masked(W, X)
    np.testing.assert_allclose(one, want, rtol=RTOL, atol=0.0)
    be.distances_chunk_rows = 100
    try:
        assert np.array_equal(_bits(be.distances_masked(W, X)), _bits(one))
    finally:
        be.distances_chunk_rows = 0
    dist, idx = be.bmu_masked(W, 2, X)
    assert np.array_equal(np.take_along_axis(one, idx, axis=1), dist)
    with pytest.raises(ValueError, match="no observed entry"):
        bad = X.copy()
        bad[3] = np.nan
        be.distances_masked(W, bad)


# ---- 4. the estimator ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from dbgsom_amd import SomVQ

    X, _ = gi.case_X("digits_f32")
    est = SomVQ(missing_values="nan", random_state=0, n_iter=8).fit(X)
    return est, X


def _agrees_with_the_search(est, X, D):
    rows = np.arange(D.shape[0])
    d1, i1 = (est._host(a) for a in est._get_winning_neurons(X, 1))
    d2, i2 = (est._host(a) for a in est._get_winning_neurons(X, 2))
    assert np.array_equal(D[rows, i1], d1) and np.array_equal(D.min(axis=1), d1)
    assert np.array_equal(np.take_along_axis(D, i2, axis=1), d2)
    assert np.array_equal(D[rows, est._host(est.predict(X))], d1)
    assert float(np.mean(D.min(axis=1))) == est.calculate_quantization_error(X)


def test_estimator_host_and_tensor(fitted):
    import torch

    est, X = fitted
    D = est.prototype_distances(X)
    assert isinstance(D, np.ndarray) and D.shape == (len(X), len(est.neurons_)) and D.dtype == np.float64
    assert est.weights_.dtype == np.float64
    _agrees_with_the_search(est, X, D)
    cols = [0, len(est.weights_) // 2, len(est.weights_) - 1]
    assert np.array_equal(D[:, cols], pd.pair_distances(X, est.weights_[cols]))
    t = torch.from_numpy(X).cuda()
    Dt = est.prototype_distances(t)
    assert isinstance(Dt, torch.Tensor) and Dt.device == t.device and Dt.dtype == torch.float64
    assert np.array_equal(_bits(Dt.cpu().numpy()), _bits(D))
    _agrees_with_the_search(est, t, Dt.cpu().numpy())
    # the README's example, as written there
    som, emb = est, t
    D = som.prototype_distances(emb)
    soft = torch.softmax(-D / D.mean(), dim=1)
    labels = som.predict(emb)
    assert torch.equal(D.gather(1, labels[:, None])[:, 0], D.min(dim=1).values)
    assert soft.shape == D.shape and torch.allclose(soft.sum(dim=1), torch.ones_like(soft[:, 0]))
    with pytest.raises(ValueError, match="features"):
        est.prototype_distances(t[:, :10])
    bad = t.clone()
    bad[4, 4] = float("nan")
    with pytest.raises(ValueError):                                   # a device tensor with NaN: refused as today
        est.prototype_distances(bad)


def test_estimator_rows_with_holes_and_sparse(fitted):
    est, X = fitted
    Xn = punch(X[:300], 0.3, 2)
    Xn[::3] = X[:300:3]                                               # every third row complete
    holes = np.isnan(Xn).any(axis=1)
    D = est.prototype_distances(Xn)
    assert np.array_equal(_bits(D[~holes]), _bits(est.prototype_distances(Xn[~holes])))
    assert np.array_equal(_bits(D[holes]), _bits(est.prototype_distances(Xn[holes])))
    np.testing.assert_allclose(D, pd.pair_distances(Xn, est.weights_), rtol=RTOL, atol=0.0)
    _agrees_with_the_search(est, Xn, D)
    Xs = sp.csr_matrix(X[:300])                                       # digits: half of the cells are zero
    assert np.array_equal(_bits(est.prototype_distances(Xs)), _bits(est.prototype_distances(X[:300])))
    assert est.prototype_distances(X[:0]).shape == (0, len(est.neurons_))
