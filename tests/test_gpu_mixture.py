"""MI355X: the map as a Gaussian mixture -- the rows kernel of csrc/mixture.hip on crafted matrices (units bit for bit,
its exact cases bit for bit against the NumPy restatement, everything else against np.longdouble within the bounds of
tests/mixture.py), the slab driver over the shape table of tests/prototype_distances.py on the exact squared matrix (and
against dbgsom_bmu on the same buffers), the context calls (chunks, rows in HBM, CSR, traffic) and both estimators.  No
test asserts on a clock."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests import device_abi as da
from tests import distortion as ds
from tests import golden_inputs as gi
from tests import mixture as mx
from tests import prototype_distances as pd

pytestmark = pytest.mark.gpu

GUARD = 8          # untouched elements in front of and behind every result


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


def _bits(a):
    """the bit patterns, every NaN as one"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


def _padded(A, ld, fill=np.nan):
    host = np.full((A.shape[0], ld), fill)
    host[:, :A.shape[1]] = A
    return da.dev(host)


class _Results:
    """unit (int64), lse (float64) of N values and q (N rows of nv values, ldq apart), every buffer filled with 0xFF
    bytes (an int64 reads -1, a float64 a NaN) with GUARD elements on either side"""

    def __init__(self, N, nv, ldq):
        import torch

        self.N, self.nv, self.ldq = N, nv, ldq
        ff = lambda n: torch.full((8 * (n + 2 * GUARD),), 0xFF, dtype=torch.uint8, device="cuda")   # noqa: E731
        self.unit, self.lse, self.q = ff(N), ff(N), ff(N * ldq)
        self.unit_ptr, self.lse_ptr = self.unit.data_ptr() + 8 * GUARD, self.lse.data_ptr() + 8 * GUARD
        self.q_ptr = self.q.data_ptr() + 8 * GUARD if nv else None

    def read(self):
        """-> (unit, lse, q); what lies around them, and behind every row of q, must still hold 0xFF bytes"""
        n, nv, ldq = self.N, self.nv, self.ldq
        unit, lse, q = (t.cpu().numpy().view(np.uint64) for t in (self.unit, self.lse, self.q))
        ff = np.uint64(0xFFFFFFFFFFFFFFFF)
        for name, a, m in (("unit", unit, n), ("lse", lse, n), ("q", q, n * ldq)):
            assert (a[:GUARD] == ff).all() and (a[GUARD + m:] == ff).all(), "a write outside " + name
        body = q[GUARD:GUARD + n * ldq].reshape(n, ldq)
        assert (body[:, nv:] == ff).all(), "a write behind a row of q"
        return (unit[GUARD:GUARD + n].view(np.int64).copy(), lse[GUARD:GUARD + n].view(np.float64).copy(),
                body[:, :nv].view(np.float64).copy() if nv else np.empty((n, 0)))


# ---- 1. dbgsom_mixture_rows on crafted matrices ---------------------------------------------------------------------
def _mixture_rows(nat, R, a, c, Y, ldr_pad=3, ldy_pad=1, ldq_pad=2):
    """the raw call with ldr = M + ldr_pad and ldy = nv + ldy_pad (NaN in the tail of every row) and ldq = nv + ldq_pad"""
    N, M = R.shape
    nv = Y.shape[1]
    rd, ad = _padded(R, M + ldr_pad), da.dev(np.asarray(a, dtype=np.float64))
    yd = _padded(Y, nv + ldy_pad) if nv else None
    out = _Results(N, nv, nv + ldq_pad)
    nat.call("dbgsom_mixture_rows", rd.data_ptr(), N, M, M + ldr_pad, ad.data_ptr(), float(c), yd.data_ptr() if nv else None,
             nv, nv + ldy_pad if nv else 0, out.unit_ptr, out.lse_ptr, out.q_ptr, nv + ldq_pad if nv else 0, da.stream())
    _sync()
    return out.read()


def _check_general(R, a, c, Y, unit, lse, q, label):
    """units bit for bit with the restatement; values within the device bound of np.longdouble; the rows the model
    defines as NaN are NaN"""
    wb, wl, wq = mx.mixture_rows(R, a, c, Y)
    assert np.array_equal(unit, wb)
    rows = mx.defined(R, a, c)
    assert np.isnan(lse[~rows]).all() and np.isnan(q[~rows]).all()
    assert np.isfinite(lse[rows]).all() and np.isfinite(q[rows]).all()
    worst = mx.check_outputs(R, a, c, Y, unit, lse, q, mx.E_DEVICE)
    print("%s: largest error / bound: lse %.3f, q %.3f; rows equal to the restatement bit for bit: %d of %d"
          % (label, worst[0], worst[1], int(np.sum(_bits(lse) == _bits(wl))), len(lse)))


@pytest.mark.skipif(not da.have_longdouble(), reason="np.longdouble has no 64-bit significand here")
@pytest.mark.parametrize("case", mx.ROWS_CASES, ids=mx.ROWS_IDS)
def test_mixture_rows_on_crafted_matrices(nat, case):
    N, M, nv, equal = case
    R, a, c, Y = mx.rows_problem(case)
    unit, lse, q = _mixture_rows(nat, R, a, c, Y)
    _check_general(R, a, c, Y, unit, lse, q, mx.ROWS_IDS[mx.ROWS_CASES.index(case)])
    if N >= mx.ROWS_KINDS:
        if equal:
            assert unit[0] == 0 and unit[1] == (63 if M > 63 else 0)     # equal maxima at lanes 0 / 63 / 64
        assert unit[2] == -1 and np.isnan(lse[2]) and np.isnan(q[2]).all()   # a row of NaN
        assert M == 1 or (unit[4] >= 0 and np.isnan(lse[4]) and np.isnan(q[4]).all())   # one NaN r
    dense = _mixture_rows(nat, R, a, c, Y, ldr_pad=0, ldy_pad=0, ldq_pad=0)   # contiguous rows: the same bytes
    assert np.array_equal(dense[0], unit) and np.array_equal(_bits(dense[1]), _bits(lse))
    assert np.array_equal(_bits(dense[2]), _bits(q))


@pytest.mark.parametrize("case", [(5, 65, 3), (9, 300, 16), (4, 257, 1), (1, 1, 2), (5, 1025, 0)],
                         ids=["N5-M65-V3", "N9-M300-V16", "N4-M257-V1", "N1-M1-V2", "N5-M1025-V0"])
def test_exact_cases_bit_for_bit(nat, case):
    N, M, nv = case
    rng = np.random.default_rng(M + nv)
    R = rng.random((N, M)) * 10.0 + 1e-3
    a = np.full(M, -np.log(M))
    Y = rng.normal(size=(M, nv))
    for c in (0.0, mx.underflow_c(R)):       # every s_j = 1; every s_j but the winner's = 0
        unit, lse, q = _mixture_rows(nat, R, a, c, Y)
        wb, wl, wq, S, Q, T = mx.mixture_rows(R, a, c, Y, parts=True)
        assert (S == (float(M) if c == 0.0 else 1.0)).all()
        assert np.array_equal(unit, wb) and np.array_equal(_bits(lse), _bits(wl)) and np.array_equal(_bits(q), _bits(wq))
        if c:
            assert np.array_equal(unit, np.argmin(R, axis=1)) and np.array_equal(_bits(lse), _bits(T))
            assert np.array_equal(_bits(q), _bits(Y[unit]))
    for c in (0.0, 0.7, mx.underflow_c(R)):  # Y all ones: q = 1
        if nv:
            assert (_mixture_rows(nat, R, a, c, np.ones((M, nv)))[2] == 1.0).all()
    # units without mass: never the unit; all of them: (-1, NaN, NaN)
    gone = a.copy()
    gone[::2] = -np.inf
    unit, lse, q = _mixture_rows(nat, R, gone, 0.7, Y)
    if M >= 2:
        assert (unit % 2 == 1).all() and np.isfinite(lse).all()
        assert np.array_equal(unit, mx.mixture_rows(R, gone, 0.7, Y)[0])
    unit, lse, q = _mixture_rows(nat, R, np.full(M, -np.inf), 0.7, Y)
    assert (unit == -1).all() and np.isnan(lse).all() and np.isnan(q).all()


# ---- 2. dbgsom_mixture ----------------------------------------------------------------------------------------------
def _norms(nat, A, ld, off, dtype):
    import torch

    t, ptr = da.stage(A, ld, off, dtype)
    out = torch.full((A.shape[0],), float("nan"), dtype=torch.float64, device="cuda")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], A.shape[0], A.shape[1], ld, out.data_ptr(), da.stream())
    return out, t, ptr


def _mixture(nat, dtype, X, W, a, c, Y, ldx, x_off, slab_rows=0, with_bmu=False, poison=False, short=0, guarded=None):
    """dbgsom_mixture with xx / ww from dbgsom_row_sqnorms on the same buffers, ldy = nv + 1 and ldq = nv + 2 ->
    (unit, lse, q), and with with_bmu the winners of dbgsom_bmu (k = 1) on the very same buffers.  poison: the workspace
    holds NaN.  guarded: a body fill of device_abi.GuardedWorkspace -- the workspace is then exactly as large as the size
    function says, between guards that must come back intact."""
    import torch

    N, d = X.shape
    M, nv = W.shape[0], Y.shape[1]
    xx, _xt, xptr = _norms(nat, X, ldx, x_off, dtype)
    ww, _wt, wptr = _norms(nat, W, d, 0, "f64")
    ad = da.dev(np.asarray(a, dtype=np.float64))
    yd = _padded(Y, nv + 1) if nv else None
    nbytes = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, slab_rows)
    gw = None
    if guarded:
        gw = da.GuardedWorkspace(nbytes)
        gw.fill(guarded)
        wsp = gw.ptr
    else:
        ws, wsp = da.workspace(nbytes)
        if poison:
            ws.view(torch.float64)[:] = float("nan")
    out = _Results(N, nv, nv + 2)
    nat.call("dbgsom_mixture", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), ad.data_ptr(),
             float(c), yd.data_ptr() if nv else None, nv, nv + 1 if nv else 0, slab_rows, out.unit_ptr, out.lse_ptr,
             out.q_ptr, nv + 2 if nv else 0, wsp, nbytes - short, da.stream())
    search = None
    if with_bmu:
        idx = torch.full((N,), -7, dtype=torch.int64, device="cuda")
        dist = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        nat.call("dbgsom_bmu", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), 1, 0,
                 idx.data_ptr(), dist.data_ptr(), da.stream())
        _sync()
        search = idx.cpu().numpy()
    _sync()
    if gw is not None:
        assert gw.intact() == (True, True), "a write outside the workspace"
    return (out.read(), search) if with_bmu else out.read()


@pytest.mark.skipif(not da.have_longdouble(), reason="np.longdouble has no 64-bit significand here")
@pytest.mark.parametrize("i", range(len(pd.CASES)), ids=pd.CASE_IDS)
def test_mixture_over_the_shape_table(nat, i):
    case = pd.CASES[i]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    R, a, c, Y, wb, wl, wq = mx.case_reference(case, mx.case_nv(i))
    unit, lse, q = _mixture(nat, dtype, X, W, a, c, Y, d + pad, x_off, poison=True)
    _check_general(R, a, c, Y, unit, lse, q, pd.CASE_IDS[i])
    # equal priors: the MAP unit is the winner of the search on the same buffers
    R, a, c, Y, wb, wl, wq = mx.case_reference(case, 0, True)
    (unit, lse, q), search = _mixture(nat, dtype, X, W, a, c, Y, d + pad, x_off, with_bmu=True)
    assert np.array_equal(unit, wb) and np.array_equal(unit, search)


def test_three_slabs_equal_one(nat):
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = mx.SLAB_CASE
    X, W, _ = pd.case_data(mx.SLAB_CASE)
    R, a, c, Y, wb, wl, wq = mx.case_reference(mx.SLAB_CASE, 3)
    assert N == 300
    one = _mixture(nat, dtype, X, W, a, c, Y, d + pad, x_off)
    three = _mixture(nat, dtype, X, W, a, c, Y, d + pad, x_off, slab_rows=100, poison=True)
    assert np.array_equal(three[0], one[0]) and np.array_equal(one[0], wb)
    assert np.array_equal(_bits(three[1]), _bits(one[1])) and np.array_equal(_bits(three[2]), _bits(one[2]))


@pytest.mark.parametrize("slab_rows", [0, 100], ids=["one-slab", "three-slabs"])
def test_exact_size_dirty_workspace_between_guards(nat, slab_rows):
    """the workspace is dbgsom_kneighbors_workspace_bytes and not a byte more: 0xFF bytes and zeros in it give the same
    bits, and nothing in front of or behind it is written"""
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = mx.SLAB_CASE
    X, W, _ = pd.case_data(mx.SLAB_CASE)
    R, a, c, Y, wb, wl, wq = mx.case_reference(mx.SLAB_CASE, 3)
    plain = _mixture(nat, dtype, X, W, a, c, Y, d + pad, x_off, slab_rows=slab_rows)
    for fill in ("ff", "zero"):
        got = _mixture(nat, dtype, X, W, a, c, Y, d + pad, x_off, slab_rows=slab_rows, guarded=fill)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[0], wb)
        assert np.array_equal(_bits(got[1]), _bits(plain[1])) and np.array_equal(_bits(got[2]), _bits(plain[2]))


def test_short_workspace_is_enomem(nat):
    from dbgsom_amd._native import DbgsomNativeError

    case = pd.CASES[0]
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    X, W, _ = pd.case_data(case)
    R, a, c, Y, wb, wl, wq = mx.case_reference(case, 2)
    nbytes = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, 0)
    with pytest.raises(DbgsomNativeError, match="%d bytes, %d needed" % (nbytes - 1, nbytes)) as err:
        _mixture(nat, dtype, X, W, a, c, Y, d + pad, x_off, short=1)
    assert err.value.code == -3
    _sync()


# ---- 3. the context calls -------------------------------------------------------------------------------------------
def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert (got[2] is None and want[2] is None) or np.array_equal(_bits(got[2]), _bits(want[2]))


def test_host_device_and_csr_agree_bit_for_bit(nat, be):
    import torch

    rng = np.random.default_rng(64)
    Xs = sp.random(203, 64, density=0.3, format="csr", dtype=np.float32, random_state=3)
    X = Xs.toarray()
    W = rng.normal(size=(41, 64)) * 0.3
    w = rng.random(41) + 0.05
    w[::7] = 0.0
    with np.errstate(divide="ignore"):
        a = np.log(w / w.sum())
    c, Y = 0.9, rng.random((41, 5))
    before = be.sample_traffic()
    whole = be.mixture(W, a, c, Y, X)
    after = be.sample_traffic()
    assert whole[0].dtype == np.int64 and whole[1].dtype == np.float64 and whole[2].shape == (203, 5)
    assert after["x_upload_bytes"] - before["x_upload_bytes"] == X.nbytes + a.nbytes + Y.nbytes   # rows, a and Y, once
    assert after["x_upload_calls"] - before["x_upload_calls"] == 2
    assert after["x_download_bytes"] - before["x_download_bytes"] == 203 * (16 + 8 * 5)           # not N x M x 8
    if da.have_longdouble():
        R = ds.squared_matrix(X, W)
        _check_general(R, a, c, Y, whole[0], whole[1], whole[2], "context, host rows")
    be.distances_chunk_rows, be.kneighbors_slab_rows = 37, 16
    try:
        mid = be.sample_traffic()
        host = be.mixture(W, a, c, Y, X)
        assert be.sample_traffic()["x_upload_calls"] - mid["x_upload_calls"] == 6 + 1             # six chunks, a | Y once
        t = torch.from_numpy(X).cuda()
        mid = be.sample_traffic()
        dev = be.mixture(W, a, c, Y, t)
        end = be.sample_traffic()
        assert end["x_download_bytes"] == mid["x_download_bytes"]                                 # no result crossed PCIe
        assert end["x_upload_bytes"] - mid["x_upload_bytes"] == a.nbytes + Y.nbytes               # and of the way up only a | Y
        for got, dtype, shape in zip(dev, (torch.int64, torch.float64, torch.float64), ((203,), (203,), (203, 5))):
            assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
            assert tuple(got.shape) == shape
        csr = be.mixture(W, a, c, Y, Xs)
        none = be.mixture(W, a, c, None, X)
        none_dev = be.mixture(W, a, c, None, t)
    finally:
        be.distances_chunk_rows, be.kneighbors_slab_rows = 0, 0
    _same(host, whole)
    _same(tuple(v.cpu().numpy() for v in dev), whole)
    _same(csr, whole)
    assert none[2] is None and none_dev[2] is None
    assert np.array_equal(none[0], whole[0]) and np.array_equal(_bits(none[1]), _bits(whole[1]))
    assert np.array_equal(none_dev[0].cpu().numpy(), whole[0])
    assert np.array_equal(_bits(none_dev[1].cpu().numpy()), _bits(whole[1]))
    wide = torch.from_numpy((rng.normal(size=(61, 80)) * 0.5).astype(np.float32)).cuda()
    view = wide[:, 8:72]                                               # strided: ldx = 80 > d, base 32 bytes in
    _same(tuple(v.cpu().numpy() for v in be.mixture(W, a, c, Y, view)), be.mixture(W, a, c, Y, view.cpu().numpy()))
    X17 = np.ascontiguousarray(X[:, :17], dtype=np.float64)            # d = 17: padded on the way up
    _same(tuple(v.cpu().numpy() for v in be.mixture(W[:, :17], a, c, Y, torch.from_numpy(X17).cuda())),
          be.mixture(W[:, :17], a, c, Y, X17))
    for bad, msg in (((W, a[:5], c, Y, X), "log_prior must be"), ((W, a, -1.0, Y, X), "c must be >= 0"),
                     ((W, a, c, Y[:5], X), "Y must be"), ((W, a, c, np.ones((41, 17)), X), "DBGSOM_MAX_MIXTURE_VALUES")):
        with pytest.raises(ValueError, match=msg):
            be.mixture(*bad)
    lib = nat.load()
    assert lib.dbgsom_ctx_mixture_query(be._ctx, X.ctypes.data, 0, 203, 64, W.ctypes.data, 41, a.ctypes.data, c,
                                        Y.ctypes.data, 17, whole[0].ctypes.data, whole[1].ctypes.data,
                                        whole[2].ctypes.data) == -1
    assert b"DBGSOM_MAX_MIXTURE_VALUES" in lib.dbgsom_last_error()
    assert lib.dbgsom_ctx_mixture_query(be._ctx, X.ctypes.data, 0, 203, 64, W.ctypes.data, 41, a.ctypes.data, float("nan"),
                                        Y.ctypes.data, 5, whole[0].ctypes.data, whole[1].ctypes.data,
                                        whole[2].ctypes.data) == -1
    assert b"c must be >= 0" in lib.dbgsom_last_error()
    assert lib.dbgsom_ctx_mixture_query(be._ctx, X.ctypes.data, 0, 203, 64, W.ctypes.data, 41, a.ctypes.data, c, None, 5,
                                        whole[0].ctypes.data, whole[1].ctypes.data, whole[2].ctypes.data) == -1
    assert b"null pointer" in lib.dbgsom_last_error()


# ---- 4. the estimators ----------------------------------------------------------------------------------------------
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
    M, d = len(est.weights_), X.shape[1]
    t = torch.from_numpy(X).cuda()
    Xz = np.where(np.abs(X) < 1.0, 0.0, X).astype(np.float32)
    h = est.fit_mixture(X).mixture_bandwidth_
    priors = est.mixture_priors_.copy()
    dist, idx = est.kneighbors(X, 1)
    assert h == math.sqrt(math.fsum(float(v) * float(v) for v in dist[:, 0]) / (500 * d))
    assert np.array_equal(priors, np.bincount(idx[:, 0], minlength=M) / 500.0)
    assert est.fit_mixture(t).mixture_bandwidth_ == h and np.array_equal(est.mixture_priors_, priors)
    hz = est.fit_mixture(Xz).mixture_bandwidth_
    assert est.fit_mixture(sp.csr_matrix(Xz)).mixture_bandwidth_ == hz
    est.fit_mixture(X)

    logp, unit = est.sample_mixture(X)
    assert isinstance(logp, np.ndarray) and logp.shape == unit.shape == (500,)
    assert logp.dtype == np.float64 and unit.dtype == np.int64 and np.isfinite(logp).all()
    with np.errstate(divide="ignore"):
        a = np.log(priors)
    c = 1.0 / (2.0 * h * h)
    R = ds.squared_matrix(X, est.weights_)
    const = 0.5 * d * math.log(2 * math.pi * h * h)
    raw_unit, raw_lse, _ = est._engine().mixture(est.weights_, a, c, None, X)
    assert np.array_equal(raw_unit, unit) and np.array_equal(_bits(logp), _bits(raw_lse - const))
    if da.have_longdouble():
        _check_general(R, a, c, np.zeros((M, 0)), unit, raw_lse, np.empty((500, 0)), "estimator")
    assert np.array_equal(_bits(est.score_samples(X)), _bits(logp))
    value = est.calculate_log_likelihood(X)
    assert value == float(np.sum(logp)) / 500
    assert np.array_equal(est.sample_mixture(X, priors="uniform")[1], est.predict(X))

    be = est._engine()
    before = be.sample_traffic()
    logp_t, unit_t = est.sample_mixture(t)
    pos_t = est.project(t)
    assert be.sample_traffic()["x_download_bytes"] == before["x_download_bytes"]          # no download
    for got, dtype in ((logp_t, torch.float64), (unit_t, torch.int64), (pos_t, torch.float64)):
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
    assert np.array_equal(unit_t.cpu().numpy(), unit) and np.array_equal(_bits(logp_t.cpu().numpy()), _bits(logp))
    assert est.calculate_log_likelihood(t) == value                                       # the same float
    pos = est.project(X)
    nodes = np.asarray(list(est.neurons_), dtype=np.float64)
    assert pos.shape == (500, 2) and np.array_equal(_bits(pos_t.cpu().numpy()), _bits(pos))
    assert (pos >= nodes.min(axis=0) - 1e-12).all() and (pos <= nodes.max(axis=0) + 1e-12).all()
    assert np.array_equal(est.project(X, bandwidth=1e-3, priors="uniform"), nodes[est.predict(X)])
    assert np.array_equal(_bits(est.score_samples(sp.csr_matrix(Xz))), _bits(est.score_samples(Xz)))
    assert (est.posterior_mean(X, np.ones(M)) == 1.0).all()
    # the README's example, as written there
    som, emb = est, t
    som.fit_mixture(emb)
    novelty = -som.score_samples(emb)
    odd = torch.topk(novelty, 100).indices
    xy = som.project(emb)
    assert odd.shape == (100,) and tuple(xy.shape) == (500, 2)
    with pytest.raises(ValueError, match="features"):
        est.score_samples(t[:, :10])
    with pytest.raises(ValueError, match="bandwidth"):
        est.score_samples(t, bandwidth=0.0)


def test_classifier_posterior_class_shares():
    import torch

    from dbgsom_amd import SomClassifier

    X, y = gi.blobs_f32(900, 12, 3, n_centers=3)
    clf = SomClassifier(random_state=0, n_iter=20, max_neurons=30).fit(X, y)
    clf.fit_mixture(X)
    M = len(clf.weights_)
    units = clf.sample_mixture(X, priors="uniform")[1]
    onehot = np.zeros((M, 3))
    np.add.at(onehot, (units, np.searchsorted(clf.classes_, y)), 1.0)
    onehot = (onehot + 1e-3) / (onehot + 1e-3).sum(axis=1, keepdims=True)
    shares = clf.posterior_mean(X[:200], onehot)
    assert shares.shape == (200, 3)
    np.testing.assert_allclose(shares.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    shares_t = clf.posterior_mean(torch.from_numpy(X[:200]).cuda(), onehot)
    assert isinstance(shares_t, torch.Tensor) and np.array_equal(_bits(shares_t.cpu().numpy()), _bits(shares))
    assert np.array_equal(_bits(clf.posterior_mean(sp.csr_matrix(X[:200]), onehot)), _bits(shares))
    assert 0.0 <= clf.score(X, y) <= 1.0
