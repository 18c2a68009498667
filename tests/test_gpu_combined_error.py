"""MI355X: the combined error of Kaski and Lagus -- the three kernels of csrc/geodesics.hip raw against their NumPy
restatement bit for bit (edge lengths; the geodesics over the graph table of tests/combined_error.py; the rows kernel
on crafted pairs), the context calls (chunks, rows in HBM, CSR, traffic) and both estimators.  Every out-of-range index
here is one the kernels must catch without reading through it.  No test asserts on a clock."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

from tests import combined_error as ce
from tests import device_abi as da
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu

GUARD = 8          # sentinel elements in front of and behind a result


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


def _guarded(n):
    """a float64 result of n values with GUARD sentinels on either side -> (tensor, pointer to the result)"""
    t = _full((n + 2 * GUARD,), ce.SENTINEL, "float64")
    return t, t.data_ptr() + 8 * GUARD


def _read_guarded(t, n):
    a = t.cpu().numpy()
    want = _bits(np.float64(ce.SENTINEL))
    assert (_bits(a[:GUARD]) == want).all() and (_bits(a[GUARD + n:]) == want).all(), "a write outside the result"
    return a[GUARD:GUARD + n].copy()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- 1. dbgsom_edge_lengths -----------------------------------------------------------------------------------------
def _edge_lengths(nat, W, edges, ldw):
    M, d = W.shape
    host = np.full((M, ldw), np.nan)
    host[:, :d] = W
    wd, ed = da.dev(host), da.dev(np.ascontiguousarray(edges, dtype=np.int32))
    out, ptr = _guarded(len(edges))
    nat.call("dbgsom_edge_lengths", wd.data_ptr(), M, d, ldw, ed.data_ptr(), len(edges), ptr, da.stream())
    _sync()
    return _read_guarded(out, len(edges))


@pytest.mark.parametrize("d, pad", [(1, 0), (1, 3), (17, 0), (17, 3), (785, 0), (785, 7)])
def test_edge_lengths_against_the_restatement(nat, d, pad):
    rng = np.random.default_rng(d + pad)
    M = 70
    W = rng.normal(size=(M, d)) * 10.0 ** rng.integers(-3, 4, size=(M, 1))
    W[9] = W[8]
    edges = np.concatenate([rng.integers(0, M, size=(513, 2)), [[8, 9], [5, 5], [0, M - 1], [M - 1, 0]]])
    got = _edge_lengths(nat, W, edges, d + pad)
    assert np.array_equal(_bits(got), _bits(ce.edge_lengths(W, edges)))
    assert got[513] == 0.0 and got[514] == 0.0 and got[515] == got[516]
    back = _edge_lengths(nat, W, edges[:, ::-1], d + pad)
    assert np.array_equal(_bits(back), _bits(got))                    # len(a, b) == len(b, a)


@pytest.mark.parametrize("bad", [70, -1, 2 ** 31 - 1])
def test_edge_lengths_index_out_of_range(nat, bad):
    from dbgsom_amd._native import DbgsomNativeError

    W = np.random.default_rng(0).normal(size=(70, 5))
    edges = np.array([[0, 1], [2, bad], [3, 4]])
    with pytest.raises(DbgsomNativeError, match=r"outside \[0, 70\)") as err:
        _edge_lengths(nat, W, edges, 5)
    assert err.value.code == -5
    _sync()


# ---- 2. dbgsom_geodesics over the graph table -----------------------------------------------------------------------
def _geodesics(nat, M, edges, lengths, sources, ldg_pad=3):
    """the raw call: a workspace of 0xFF bytes, rows ldg = M + ldg_pad apart in a buffer of sentinels"""
    E = len(edges)
    S = M if sources is None else len(sources)
    ldg = M + ldg_pad
    ed = da.dev(np.ascontiguousarray(edges, dtype=np.int32)) if E else None
    ld = da.dev(np.ascontiguousarray(lengths, dtype=np.float64)) if E else None
    sd = None if sources is None else da.dev(np.ascontiguousarray(sources, dtype=np.int32))
    nbytes = nat.load().dbgsom_geodesics_workspace_bytes(M, E)
    assert nbytes >= 4
    ws = _full((nbytes,), 0xFF, "uint8")
    out, ptr = _guarded(S * ldg)
    nat.call("dbgsom_geodesics", _ptr(ed), _ptr(ld), E, M, _ptr(sd), S, ptr, ldg, ws.data_ptr(), nbytes, da.stream())
    _sync()
    G = _read_guarded(out, S * ldg).reshape(S, ldg)
    assert (_bits(G[:, M:]) == _bits(np.float64(ce.SENTINEL))).all(), "a write behind a row"
    return G[:, :M]


@pytest.mark.parametrize("name", ce.GRAPH_IDS)
def test_geodesics_against_the_restatement(nat, name):
    M, edges, lengths, sources, want = ce.graph(name)
    got = _geodesics(nat, M, edges, lengths, sources)
    assert np.array_equal(_bits(got), _bits(want))


def test_geodesics_of_a_source_list_with_a_repeat(nat):
    M, edges, lengths, _, want = ce.graph("holes16")
    sources = np.array([5, 200, 5, 0, 255, 34])
    got = _geodesics(nat, M, edges, lengths, sources, ldg_pad=0)
    assert np.array_equal(_bits(got), _bits(want[sources]))
    assert np.array_equal(_bits(got[0]), _bits(got[2]))
    everything = _geodesics(nat, M, edges, lengths, None, ldg_pad=0)   # contiguous rows: the same bytes
    assert np.array_equal(_bits(everything), _bits(want))


@pytest.mark.parametrize("bad", [np.nan, -1.0, -np.inf])
def test_geodesics_refuse_a_bad_length(nat, bad):
    M, edges, lengths, _, _ = ce.graph("duplicates")
    lengths = lengths.copy()
    lengths[11] = bad
    with pytest.raises(ValueError, match=r"dbgsom_geodesics failed \(-1\): .*NaN or negative"):   # DBGSOM_EINVAL
        _geodesics(nat, M, edges, lengths, None)
    _sync()


def test_geodesics_index_out_of_range(nat):
    from dbgsom_amd._native import DbgsomNativeError

    M, edges, lengths, _, _ = ce.graph("duplicates")
    for bad in (M, -1, 2 ** 31 - 1):
        for col in (0, 1):
            e = edges.copy()
            e[7, col] = bad
            with pytest.raises(DbgsomNativeError, match=r"outside \[0, 30\)") as err:
                _geodesics(nat, M, e, lengths, None)
            assert err.value.code == -5
        with pytest.raises(DbgsomNativeError, match=r"outside \[0, 30\)") as err:
            _geodesics(nat, M, edges, lengths, np.array([3, bad, 4]))
        assert err.value.code == -5
    _sync()


# ---- 3. dbgsom_combined_error_rows on crafted pairs -----------------------------------------------------------------
def _rows(nat, idx2, dist, G, ldg_pad=2):
    N, M = len(idx2), len(G)
    host = np.full((M, M + ldg_pad), np.nan)
    host[:, :M] = G
    gd, idd, dd = da.dev(host), da.dev(np.ascontiguousarray(idx2, dtype=np.int64)), da.dev(dist)
    out, ptr = _guarded(N)
    nat.call("dbgsom_combined_error_rows", idd.data_ptr(), dd.data_ptr(), dist.shape[1], N, gd.data_ptr(), M + ldg_pad, M,
             ptr, da.stream())
    _sync()
    return _read_guarded(out, N)


@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("ldd", [2, 5])
def test_rows_kernel_on_crafted_pairs(nat, N, ldd):
    rng = np.random.default_rng(N + ldd)
    M = 37
    G = rng.random((M, M)) * 10.0 ** rng.integers(-3, 4, size=(M, M))
    np.fill_diagonal(G, 0.0)
    G[3, 4] = G[4, 3] = np.inf
    idx2 = rng.integers(0, M, size=(N, 2))
    dist = rng.random((N, ldd)) * 3.0
    special = [(-1, 2), (2, -1), (-1, -1), (5, 5), (3, 4), (M - 1, 0)]
    for r, pair in enumerate(special[N == 1 and ldd % len(special):][:N]):
        idx2[r] = pair
    got = _rows(nat, idx2, dist, G)
    want = ce.combined_error_rows(idx2, dist[:, 0], G)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got), (idx2 < 0).any(axis=1))
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok]))
    if N > 1:
        assert np.isnan(got[:3]).all() and got[3] == dist[3, 0] and got[4] == np.inf


def test_rows_kernel_index_out_of_range(nat):
    from dbgsom_amd._native import DbgsomNativeError

    G = np.ones((37, 37))
    for bad in (37, -2, 2 ** 40):
        for col in (0, 1):
            idx2 = np.zeros((300, 2), dtype=np.int64)
            idx2[271, col] = bad
            with pytest.raises(DbgsomNativeError, match=r"outside \[0, 37\)") as err:
                _rows(nat, idx2, np.ones((300, 2)), G)
            assert err.value.code == -5
    _sync()


# ---- 4. the context calls -------------------------------------------------------------------------------------------
def _sheet(rows, cols, d, seed, N, dtype=np.float32):
    """prototypes of a rows x cols sheet, its edges (int32) and N rows scattered around the prototypes"""
    rng = np.random.default_rng(seed)
    M = rows * cols
    W = rng.normal(size=(M, d)) * 1.5
    X = (W[rng.integers(0, M, size=N)] + rng.normal(size=(N, d)) * 0.7).astype(dtype)
    return W, ce.lattice_edges(rows, cols), X


def test_backend_geodesics(be):
    W, edges, _ = _sheet(9, 7, 17, 1, 1)
    before = be.sample_traffic()
    G = be.geodesics(W, edges)
    after = be.sample_traffic()
    assert G.shape == (63, 63) and G.dtype == np.float64
    assert np.array_equal(_bits(G), _bits(ce.geodesics(63, edges, ce.edge_lengths(W, edges))))
    assert after["x_download_bytes"] - before["x_download_bytes"] == 63 * 63 * 8
    assert after["x_upload_bytes"] - before["x_upload_bytes"] == edges.nbytes
    alone = be.geodesics(W, np.empty((0, 2), dtype=np.int64))          # no edges: every unit is a component
    assert np.array_equal(np.isinf(alone), ~np.eye(63, dtype=bool)) and (np.diag(alone) == 0.0).all()
    with pytest.raises(ValueError, match=r"outside \[0, 63\)"):
        be.geodesics(W, np.array([[0, 63]]))


def test_host_path_in_chunks(be):
    W, edges, X = _sheet(6, 7, 784, 2, 300)
    want_e, want_u = ce.combined_error(X, W, edges)
    before = be.sample_traffic()
    e, units = be.combined_error(W, edges, X)
    after = be.sample_traffic()
    assert e.dtype == np.float64 and units.dtype == np.int64 and e.shape == (300,) and units.shape == (300, 2)
    assert np.array_equal(units, want_u) and np.array_equal(_bits(e), _bits(want_e))
    assert after["x_upload_bytes"] - before["x_upload_bytes"] == X.nbytes + edges.nbytes      # the rows and the edges, once
    assert after["x_upload_calls"] - before["x_upload_calls"] == 2
    assert after["x_download_bytes"] - before["x_download_bytes"] == 300 * 24
    be.distances_chunk_rows = 37
    try:
        e3, u3 = be.combined_error(W, edges, X)
        assert be.sample_traffic()["x_upload_calls"] - after["x_upload_calls"] == 9 + 1       # nine chunks, the edges once
    finally:
        be.distances_chunk_rows = 0
    assert np.array_equal(u3, units) and np.array_equal(_bits(e3), _bits(e))
    X64 = np.ascontiguousarray(X[:, :17], dtype=np.float64)           # d = 17: padded on the way up
    e17, u17 = be.combined_error(W[:, :17], edges, X64)
    w17 = ce.combined_error(X64, W[:, :17], edges)
    assert np.array_equal(u17, w17[1]) and np.array_equal(_bits(e17), _bits(w17[0]))
    cut = edges[(edges // 7 != 3).all(axis=1)]                          # row 3 of the sheet loses every edge
    ec, uc = be.combined_error(W, cut, X)
    wc = ce.combined_error(X, W, cut)
    assert np.array_equal(uc, units) and np.array_equal(_bits(ec), _bits(wc[0])) and np.isposinf(ec).any()
    with pytest.raises(ValueError, match="at least two prototypes"):
        be.combined_error(W[:1], np.empty((0, 2), dtype=np.int32), X)
    with pytest.raises(ValueError, match="feature mismatch"):
        be.combined_error(W[:, :5], edges, X)


def test_device_path_equals_host_path(be):
    import torch

    rng = np.random.default_rng(7)
    W48, edges, X48 = _sheet(5, 8, 48, 3, 301)
    W17, _, X17 = _sheet(5, 8, 17, 4, 301, np.float64)
    wide = torch.from_numpy((rng.normal(size=(301, 80)) * 2.0).astype(np.float32)).cuda()
    view = wide[:, 8:56]                                              # strided: ldx = 80 > d, base 32 bytes in
    for W, host, t in ((W48, X48, torch.from_numpy(X48).cuda()),      # borrowed where it lies
                       (W17, X17, torch.from_numpy(X17).cuda()),      # pad-copied on the device
                       (W48, view.cpu().numpy(), view)):
        want_e, want_u = be.combined_error(W, edges, host)
        before = be.sample_traffic()
        e, units = be.combined_error(W, edges, t)
        after = be.sample_traffic()
        assert after["x_download_bytes"] == before["x_download_bytes"]                    # no result crossed PCIe
        assert after["x_upload_bytes"] - before["x_upload_bytes"] == edges.nbytes         # and of the way up only the edges
        for got, dtype, shape in ((e, torch.float64, (301,)), (units, torch.int64, (301, 2))):
            assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
            assert tuple(got.shape) == shape
        assert np.array_equal(units.cpu().numpy(), want_u) and np.array_equal(_bits(e.cpu().numpy()), _bits(want_e))
        w = ce.combined_error(np.ascontiguousarray(host), W, edges)
        assert np.array_equal(want_u, w[1]) and np.array_equal(_bits(want_e), _bits(w[0]))


def test_csr_equals_dense(be):
    rng = np.random.default_rng(64)
    Xs = sp.random(203, 64, density=0.3, format="csr", dtype=np.float32, random_state=3)
    W = rng.normal(size=(42, 64)) * 0.5
    edges = ce.lattice_edges(6, 7)
    dense_e, dense_u = be.combined_error(W, edges, Xs.toarray())
    be.distances_chunk_rows = 64
    try:
        e, units = be.combined_error(W, edges, Xs)
    finally:
        be.distances_chunk_rows = 0
    assert np.array_equal(units, dense_u) and np.array_equal(_bits(e), _bits(dense_e))
    w = ce.combined_error(Xs.toarray(), W, edges)
    assert np.array_equal(units, w[1]) and np.array_equal(_bits(e), _bits(w[0]))


def test_the_query_search_at_k2_is_the_all_pairs_one(be):
    """The query driver takes its filtered form at k = 1 only: no shape exists at which query_filter_applies(N, d, M, 2)
    holds, so a map large enough for the filter runs the all-pairs search here -- against the oracle."""
    from dbgsom_amd.backend import HipBackend

    N, d, rows, cols = 8192, 64, 18, 20
    M = rows * cols
    auto = HipBackend(0, algorithm="filtered")
    try:
        assert M >= auto.FILTER_MIN_PROTOTYPES and d <= auto.FILTER_MAX_FEATURES
        assert not auto.query_filter_applies(N, d, M, 2)
        assert not auto.query_filter_applies(30_000, 200, M, 2)          # the shape of the resident pruning test
        assert not auto.query_filter_applies(10 ** 6, 784, 1024, 2)
        W, edges, X = _sheet(rows, cols, d, 5, N)
        e, units = auto.combined_error(W, edges, X)
    finally:
        auto.release()
    want_e, want_u = ce.combined_error(X, W, edges)
    assert np.array_equal(units, want_u) and np.array_equal(_bits(e), _bits(want_e))


# ---- 5. the estimators ----------------------------------------------------------------------------------------------
def _both(kind):
    """an estimator fitted on the CPU stand-in and its twin on the GPU backend carrying the same fitted state"""
    from dbgsom_amd import SomClassifier, SomVQ

    X, y = gi.blobs_f32(1500, 24, 5, n_centers=12)
    kw = dict(random_state=0, n_iter=20, max_neurons=40, spreading_factor=0.9)
    if kind == "vq":
        host = SomVQ(backend=ce.CombinedErrorOracleBackend(), **kw).fit(X)
    else:
        host = SomClassifier(backend=ce.CombinedErrorOracleBackend(), **kw).fit(X, y % 3)
    dev = pickle.loads(pickle.dumps(host))
    dev.backend = None
    return host, dev, X[:500]


@pytest.mark.parametrize("kind", ["vq", "classifier"])
def test_estimator_host_tensor_and_csr(kind):
    import torch

    from dbgsom_amd.backend import HipBackend

    host, est, X = _both(kind)
    assert isinstance(est._engine(), HipBackend)
    M = len(est.weights_)
    assert M >= 12
    G = est.prototype_geodesics()
    assert G.shape == (M, M) and np.array_equal(_bits(G), _bits(host.prototype_geodesics()))
    want_e, want_u = host.sample_combined_error(X)
    e, units = est.sample_combined_error(X)
    assert isinstance(e, np.ndarray) and isinstance(units, np.ndarray)
    assert e.shape == (500,) and units.shape == (500, 2) and e.dtype == np.float64 and units.dtype == np.int64
    assert np.array_equal(units, want_u) and np.array_equal(_bits(e), _bits(want_e))
    if kind == "vq":
        assert np.array_equal(units[:, 0], est.predict(X))
    value = est.calculate_combined_error(X)
    assert value == float(np.sum(e)) / 500 == host.calculate_combined_error(X)
    assert value >= est.calculate_quantization_error(X)

    t = torch.from_numpy(X).cuda()
    be = est._engine()
    before = be.sample_traffic()
    e_t, units_t = est.sample_combined_error(t)
    assert be.sample_traffic()["x_download_bytes"] == before["x_download_bytes"]          # no download
    for got, dtype in ((e_t, torch.float64), (units_t, torch.int64)):
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == dtype
    assert np.array_equal(units_t.cpu().numpy(), units) and np.array_equal(_bits(e_t.cpu().numpy()), _bits(e))
    if kind == "vq":
        assert torch.equal(units_t[:, 0], est.predict(t))

    Xz = np.where(np.abs(X) < 1.0, 0.0, X).astype(np.float32)
    e_s, units_s = est.sample_combined_error(sp.csr_matrix(Xz))
    e_d, units_d = est.sample_combined_error(Xz)
    assert np.array_equal(units_s, units_d) and np.array_equal(_bits(e_s), _bits(e_d))
    assert np.array_equal(_bits(e_d), _bits(host.sample_combined_error(Xz)[0]))
    # a host array, a tensor and CSR rows of the same data: the same float
    three = (est.calculate_combined_error(Xz), est.calculate_combined_error(torch.from_numpy(Xz).cuda()),
             est.calculate_combined_error(sp.csr_matrix(Xz)))
    assert three[0] == three[1] == three[2] == host.calculate_combined_error(Xz)

    with pytest.raises(ValueError, match="features"):
        est.sample_combined_error(t[:, :10])
    empty_e, empty_u = est.sample_combined_error(X[:0])
    assert empty_e.shape == (0,) and empty_u.shape == (0, 2)
