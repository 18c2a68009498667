"""CPU: the combined error of Kaski and Lagus -- the NumPy restatement of csrc/geodesics.hip against scipy's Dijkstra bit
for bit on the whole graph table, what every graph of the table claims, the estimator plumbing on a CPU stand-in
backend, every refusal by its message, and the argument errors of the new ABI calls as status codes."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components, shortest_path
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd.backend import HotPathBackend
from tests import combined_error as ce
from tests import golden_inputs as gi
from tests.test_missing_cpu import punch


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _adjacency(M, edges, lengths):
    u, v, l = ce.directed(edges, lengths)
    keep = l < np.inf
    return sp.csr_matrix((np.ones(keep.sum()), (u[keep], v[keep])), shape=(M, M))


# ---- the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ce.GRAPH_IDS)
def test_restatement_equals_scipy_dijkstra(name):
    M, edges, lengths, sources, G = ce.graph(name)
    S = M if sources is None else len(sources)
    assert G.shape == (S, M)
    want = ce.scipy_rows(M, edges, lengths, sources)
    assert np.array_equal(_bits(G), _bits(want))
    src = np.arange(M) if sources is None else sources
    assert (G[np.arange(S), src] == 0.0).all() and not np.isnan(G).any() and (G >= 0.0).all()


def test_graphs_reach_what_they_claim():
    g = {name: ce.graph(name) for name in ce.GRAPH_IDS}
    assert g["single"][0] == 1 and len(g["single"][1]) == 0 and g["pair"][0] == 2 and len(g["pair"][1]) == 1
    # the path needs M - 1 = 299 rounds, the bound of the loop
    M, edges, lengths, _, _ = g["path300"]
    assert ce.geodesics(M, edges, lengths, [0], want_rounds=True)[1] == 299 == M - 1
    # holes and several components: isolated units, and two large pieces
    M, edges, lengths, _, G = g["holes16"]
    n, label = connected_components(_adjacency(M, edges, lengths), directed=False)
    assert n == 6 and sorted(np.bincount(label))[-2:] == [95, 157] and np.isinf(G).any()
    assert np.array_equal(np.isinf(G), label[:, None] != label[None, :])
    # the star: one unit of degree 2099
    M, edges, _, _, G = g["star"]
    assert np.bincount(edges.ravel()).max() == 2099 == M - 1
    # the cycle: the shortest path between the ends of the long edge has 199 hops, breadth-first depth 1
    M, edges, lengths, _, G = g["cycle200"]
    assert G[0, 199] == 199.0 == G[199, 0] and lengths[199] == 1e6 and tuple(edges[199]) == (199, 0)
    assert shortest_path(_adjacency(M, edges, lengths), unweighted=True)[0, 199] == 1
    assert ce.geodesics(M, edges, lengths, [0], want_rounds=True)[1] == 199
    # a zero-length edge between duplicates: their rows are equal
    M, edges, lengths, _, G = g["duplicates"]
    zero = np.flatnonzero(lengths == 0.0)
    assert len(zero) == 1 and sorted(edges[zero[0]]) == [7, 8] and G[7, 8] == 0.0 and np.array_equal(G[7], G[8])
    # self-loops and repeated edges: the shortest of the repeats counts, a loop changes nothing
    M, edges, lengths, _, G = g["loops_and_repeats"]
    assert (edges[:, 0] == edges[:, 1]).sum() == 3 and G[0, 1] == 2.0 and G[1, 2] == 0.75 and G[0, 4] == 4.75 < 9.0
    assert len({tuple(sorted(e)) for e in edges.tolist()}) < len(edges)
    # +inf connects nothing
    M, edges, lengths, _, G = g["inf_edge"]
    assert np.isinf(lengths).sum() == 1 and np.isinf(G[:5, 5:]).all() and np.isfinite(G[:5, :5]).all()
    # 300 decades on one path
    M, edges, lengths, _, G = g["wide_range"]
    assert lengths[0] == 1e-150 and lengths[-1] == 1e150 and np.isfinite(G).all()
    assert G[0, 1] == 1e-150 and G[30, 29] == 1e150 and G[0, 14] < 1.0 < G[0, 16] and G[0, 30] >= 1e150
    # the strides of the kernel's loop over the edges, and the LDS threshold
    for nt, names in ((ce.NT_SMALL, ("stride255", "stride256", "stride257")),
                      (ce.NT_LARGE, ("stride1023", "stride1024", "stride1025"))):
        assert [len(g[n][1]) for n in names] == [nt - 1, nt, nt + 1]
        assert all((g[n][0] <= ce.LDS_SMALL_M) == (nt == ce.NT_SMALL) for n in names)
    assert g["lds64k"][0] * 8 == 65536 and g["lds64k+1"][0] == ce.LDS_SMALL_M + 1
    M, _, _, sources, G = g["max"]
    assert M == ce.MAX_M == _native.MAX_PROTOTYPES and list(sources) == [0, 8000, 15999] and np.isfinite(G).all()


def test_edge_lengths_are_symmetric_and_sequential():
    rng = np.random.default_rng(0)
    W = rng.normal(size=(40, 785)) * 10.0 ** rng.integers(-3, 4, size=(40, 1))
    edges = rng.integers(0, 40, size=(300, 2))
    ab, ba = ce.edge_lengths(W, edges), ce.edge_lengths(W, edges[:, ::-1])
    assert np.array_equal(_bits(ab), _bits(ba))
    for e in (0, 17, 299):                        # the definition, scalar by scalar
        s = 0.0
        for k in range(785):
            t = W[edges[e, 0], k] - W[edges[e, 1], k]
            p = t * t
            s = s + p
        assert ab[e] == np.sqrt(s)
    exact = np.sqrt(np.sum((W[edges[:, 0]].astype(np.longdouble) - W[edges[:, 1]]) ** 2, axis=1))
    np.testing.assert_allclose(ab, exact.astype(np.float64), rtol=(785 + 4) * ce.U)
    assert (ce.edge_lengths(W, [[3, 3]]) == 0.0).all()


def test_rows_fold_from_their_own_end():
    """G[s, t] and G[t, s] add the same lengths from different ends: within hops * u * G, and not equal everywhere"""
    for name in ("path300", "holes16", "duplicates"):
        M, edges, lengths, _, G = ce.graph(name)
        hops = shortest_path(_adjacency(M, edges, lengths), unweighted=True)
        fin = np.isfinite(G)
        assert np.array_equal(fin, fin.T)
        bound = np.where(fin, hops, 0.0) * ce.U * np.where(fin, G, 0.0)
        diff = np.abs(np.where(fin, G, 0.0) - np.where(fin, G, 0.0).T)
        assert (diff <= bound).all()
        assert (diff > 0).any()


def test_combined_error_rows_restated():
    G = np.array([[0.0, 2.0, np.inf], [2.5, 0.0, 1.0], [np.inf, 1.0, 0.0]])
    idx2 = np.array([[0, 1], [1, 0], [0, 2], [-1, 1], [1, -1], [2, 2]])
    e = ce.combined_error_rows(idx2, np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.5]), G)
    assert e[0] == 3.0 and e[1] == 3.5 and e[2] == np.inf and np.isnan(e[3]) and np.isnan(e[4]) and e[5] == 0.5


# ---- estimator plumbing on the stand-in -----------------------------------------------------------------------------
FIT_KW = dict(random_state=0, n_iter=15, max_neurons=20)


@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=ce.CombinedErrorOracleBackend(), **FIT_KW).fit(X)
    return est, X


def _edges_of(est):
    index = {n: i for i, n in enumerate(est.neurons_)}
    return np.array([(index[a], index[b]) for a, b in est.som_.edges], dtype=np.int64).reshape(-1, 2)


def _check_estimator(est, X):
    M = len(est.weights_)
    edges = _edges_of(est)
    G = est.prototype_geodesics()
    assert G.shape == (M, M) and G.dtype == np.float64
    assert np.array_equal(_bits(G), _bits(ce.geodesics(M, edges, ce.edge_lengths(est.weights_, edges))))
    e, units = est.sample_combined_error(X)
    n = len(X)
    assert e.shape == (n,) and e.dtype == np.float64 and units.shape == (n, 2) and units.dtype == np.int64
    d2, idx2 = ce.two_nearest(X, est.weights_)
    assert np.array_equal(units, idx2)
    assert (e >= d2[:, 0]).all()
    assert np.array_equal(_bits(e), _bits(d2[:, 0] + G[units[:, 0], units[:, 1]]))
    adjacent = np.zeros((M, M), dtype=bool)
    adjacent[edges[:, 0], edges[:, 1]] = adjacent[edges[:, 1], edges[:, 0]] = True
    nb = adjacent[units[:, 0], units[:, 1]]
    assert nb.any()
    direct = ce.edge_lengths(est.weights_, units[nb])
    # lattice neighbours: the edge itself is the shortest way (the triangle inequality of the input space)
    assert np.array_equal(_bits(e[nb]), _bits(d2[nb, 0] + direct))
    value = est.calculate_combined_error(X)
    assert value == float(np.sum(e)) / n
    assert value >= est.calculate_quantization_error(X) > 0.0
    return e, units


def test_sample_and_mean_on_the_stand_in(fitted):
    est, X = fitted
    be = est._engine()
    be.combined_rows, be.combined_edges = [], []
    e, units = _check_estimator(est, X[:90])
    assert np.array_equal(units[:, 0], est.predict(X[:90]))
    assert be.combined_rows[0] == 90 and np.array_equal(be.combined_edges[0], _edges_of(est))
    assert be.combined_edges[0].dtype == np.int32
    Xi = np.rint(X[:20]).astype(np.int64)                 # anything but float32 becomes float64, as for predict
    assert np.array_equal(est.sample_combined_error(Xi)[1][:, 0], est.predict(Xi))


def test_classifier_inherits_it():
    X, y = gi.blobs_f32(300, 5, 4, n_centers=3)
    clf = SomClassifier(backend=ce.CombinedErrorOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    _check_estimator(clf, X[:60])


def test_after_dead_units_and_a_pickle():
    X, _ = gi.case_X("blobs_dead")
    est = SomVQ(backend=ce.CombinedErrorOracleBackend(), **gi.EST_KWARGS["blobs_dead"]).fit(X)
    e, units = _check_estimator(est, X[:50])
    G = est.prototype_geodesics()
    clone = pickle.loads(pickle.dumps(est))
    clone.backend = ce.CombinedErrorOracleBackend()
    e2, units2 = clone.sample_combined_error(X[:50])
    assert np.array_equal(units2, units) and np.array_equal(_bits(e2), _bits(e))
    assert np.array_equal(_bits(clone.prototype_geodesics()), _bits(G))
    assert np.array_equal(clone._engine().combined_edges[0], est._engine().combined_edges[-1])
    assert clone.calculate_combined_error(X[:50]) == est.calculate_combined_error(X[:50])


def test_a_map_cut_in_two_has_an_infinite_error(fitted):
    est, X = fitted
    clone = pickle.loads(pickle.dumps(est))
    clone.backend = ce.CombinedErrorOracleBackend()
    xs = sorted(n[0] for n in clone.neurons_)
    cut = xs[len(xs) // 2]
    assert xs[0] < cut
    clone.som_.remove_edges_from([(a, b) for a, b in clone.som_.edges if (a[0] < cut) != (b[0] < cut)])
    G = clone.prototype_geodesics()
    side = np.array([n[0] < cut for n in clone.neurons_])
    assert np.isinf(G[side][:, ~side]).all() and np.isinf(G[~side][:, side]).all()
    e, units = clone.sample_combined_error(X)
    across = side[units[:, 0]] != side[units[:, 1]]
    assert across.any() and not across.all()
    assert np.isposinf(e[across]).all() and np.isfinite(e[~across]).all()
    assert clone.calculate_combined_error(X) == np.inf
    assert np.isfinite(est.calculate_combined_error(X))


def test_sparse_equals_dense(fitted):
    est, X = fitted
    Xs = np.where(np.abs(X[:120]) < 2.0, 0.0, X[:120]).astype(np.float32)
    e, units = est.sample_combined_error(Xs)
    for fmt in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        got = est.sample_combined_error(fmt(Xs))
        assert np.array_equal(_bits(got[0]), _bits(e)) and np.array_equal(got[1], units)
        assert est.calculate_combined_error(fmt(Xs)) == est.calculate_combined_error(Xs)


def test_empty_input(fitted):
    est, X = fitted
    be = est._engine()
    be.combined_rows = []
    for empty in (X[:0], np.empty((0, X.shape[1]))):
        e, units = est.sample_combined_error(empty)            # as kneighbors: empty results, no launch
        assert e.shape == (0,) and units.shape == (0, 2) and e.dtype == np.float64 and units.dtype == np.int64
        with pytest.raises(ValueError, match="0 sample"):      # as calculate_quantization_error: no mean of nothing
            est.calculate_combined_error(empty)
    assert be.combined_rows == []


def test_refusals_and_their_messages(fitted):
    est, X = fitted
    for name in ("sample_combined_error", "calculate_combined_error"):
        with pytest.raises(NotFittedError):
            getattr(SomVQ(backend=ce.CombinedErrorOracleBackend()), name)(X)
    with pytest.raises(NotFittedError):
        SomVQ(backend=ce.CombinedErrorOracleBackend()).prototype_geodesics()
    for call in (est.sample_combined_error, est.calculate_combined_error):
        with pytest.raises(ValueError, match="X has 5 features, but SomVQ is expecting 8 features as input"):
            call(X[:10, :5])
        with pytest.raises(ValueError, match="features"):
            call(sp.csr_matrix(X[:10, :5]))
        with pytest.raises(ValueError, match="features"):
            call(np.empty((0, 3)))
        with pytest.raises(ValueError, match="NaN"):
            call(punch(X[:40], 0.3, 3))
        with pytest.raises(ValueError, match="[Ii]nf"):
            call(np.where(np.isnan(punch(X[:40], 0.3, 3)), np.inf, X[:40]))
    for missing in ("nan", "nan-fit"):
        holes = SomVQ(backend=ce.CombinedErrorOracleBackend(), missing_values=missing, **FIT_KW).fit(X)
        assert holes.sample_combined_error(X[:10])[0].shape == (10,)
        for call in (holes.sample_combined_error, holes.calculate_combined_error):
            with pytest.raises(ValueError, match="impute them first"):
                call(punch(X[:40], 0.3, 3))
    for metric, label in (("manhattan", "Manhattan"), ("cosine", "cosine")):
        other = SomVQ(backend=ce.CombinedErrorOracleBackend(), **FIT_KW)
        other.__dict__.update(est.__dict__)
        other.metric = metric
        for call in (other.sample_combined_error, other.calculate_combined_error):
            with pytest.raises(ValueError, match=r"metric='%s' \(%s\) does not support .*combined_error.*Euclidean"
                                                 % (metric, label)):
                call(X[:10])
    small = SomVQ(backend=ce.CombinedErrorOracleBackend(), **FIT_KW)
    small.__dict__.update(est.__dict__)
    small.weights_ = est.weights_[:1]
    for call in (small.sample_combined_error, small.calculate_combined_error):
        with pytest.raises(ValueError, match="at least two prototypes, this one has 1"):
            call(X[:10])


def test_base_backend_has_neither():
    with pytest.raises(NotImplementedError):
        HotPathBackend().geodesics(np.zeros((2, 3)), np.array([[0, 1]]))
    with pytest.raises(NotImplementedError):
        HotPathBackend().combined_error(np.zeros((2, 3)), np.array([[0, 1]]), np.zeros((4, 3)))
    for name in ("geodesics", "combined_error"):
        doc = getattr(HotPathBackend, name).__doc__
        assert "fold" in doc or "G[b1_i, b2_i]" in doc


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()   # noqa: E731
    one = 256                               # any non-null aligned address: argument errors come before any device work
    big = _native.MAX_PROTOTYPES + 1

    lens = lambda M=5, d=4, ldw=4, E=3, w=one, e=one, out=one: lib.dbgsom_edge_lengths(w, M, d, ldw, e, E, out, None)   # noqa: E731
    assert lens(M=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert lens(M=big) == -1 and b"MAX_PROTOTYPES" in err()
    assert lens(ldw=3) == -1 and b"ldw" in err()
    assert lens(d=0, ldw=0) == -1 and b"shape" in err()
    assert lens(E=-1) == -1 and b"E" in err()
    for null in ("w", "e", "out"):
        assert lens(**{null: None}) == -1 and b"null pointer" in err()
    assert lens(out=260) == -1 and b"aligned" in err()
    assert lens(E=0, w=None, e=None, out=None) == 0          # no edges: nothing to do, nothing dereferenced

    need = lib.dbgsom_geodesics_workspace_bytes(5, 3)
    assert need >= 4 and lib.dbgsom_geodesics_workspace_bytes(_native.MAX_PROTOTYPES, 1 << 20) >= 4
    assert lib.dbgsom_geodesics_workspace_bytes(0, 3) == 0 and lib.dbgsom_geodesics_workspace_bytes(big, 3) == 0
    assert lib.dbgsom_geodesics_workspace_bytes(5, -1) == 0
    geo = lambda E=3, M=5, S=5, ldg=5, e=one, l=one, src=None, g=one, w=one, ws=need: (   # noqa: E731
        lib.dbgsom_geodesics(e, l, E, M, src, S, g, ldg, w, ws, None))
    assert geo(M=0, S=0, ldg=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert geo(M=big, S=big, ldg=big) == -1 and b"MAX_PROTOTYPES" in err()
    assert geo(E=-1) == -1 and b"E" in err()
    assert geo(S=-1, src=one) == -1 and b"S" in err()
    assert geo(S=3) == -1 and b"S must be M" in err()
    assert geo(ldg=4) == -1 and b"ldg" in err()
    for null in ("e", "l", "g"):
        assert geo(**{null: None}) == -1 and b"null pointer" in err()
    assert geo(w=None) == -1 and b"null pointer" in err()
    assert geo(g=260) == -1 and b"aligned" in err()
    assert geo(ws=need - 1) == -3 and (b"%d bytes, %d needed" % (need - 1, need)) in err()
    assert geo(w=one + 8) == -1 and b"256-byte aligned" in err()

    rows = lambda N=10, M=5, ldd=2, ldg=5, i=one, d=one, g=one, e=one: (   # noqa: E731
        lib.dbgsom_combined_error_rows(i, d, ldd, N, g, ldg, M, e, None))
    assert rows(M=0, ldg=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert rows(M=big, ldg=big) == -1 and b"MAX_PROTOTYPES" in err()
    assert rows(N=-1) == -1 and b"shape" in err()
    assert rows(ldd=0) == -1 and b"ldd" in err()
    assert rows(ldg=4) == -1 and b"ldg" in err()
    for null in ("i", "d", "g", "e"):
        assert rows(**{null: None}) == -1 and b"null pointer" in err()
    assert rows(e=260) == -1 and b"aligned" in err()
    assert rows(N=0, i=None, d=None, g=None, e=None) == 0

    W = np.zeros((5, 4))
    edges = np.array([[0, 1], [1, 2]], dtype=np.int32)
    out = np.zeros(64)
    w, ed = W.ctypes.data, edges.ctypes.data
    assert lib.dbgsom_ctx_geodesics(None, w, 5, 4, ed, 2, one) == -1 and b"null context" in err()
    ctx = out.ctypes.data                    # (no context: the checks below come before it is touched)
    assert lib.dbgsom_ctx_geodesics(ctx, w, 0, 4, ed, 2, one) == -1 and b"MAX_PROTOTYPES" in err()
    assert lib.dbgsom_ctx_geodesics(ctx, w, big, 4, ed, 2, one) == -1 and b"MAX_PROTOTYPES" in err()
    assert lib.dbgsom_ctx_geodesics(ctx, w, 5, 4, ed, -1, one) == -1 and b"E" in err()
    assert lib.dbgsom_ctx_geodesics(ctx, None, 5, 4, ed, 2, one) == -1 and b"null pointer" in err()
    assert lib.dbgsom_ctx_geodesics(ctx, w, 5, 4, None, 2, one) == -1 and b"null pointer" in err()
    assert lib.dbgsom_ctx_geodesics(ctx, w, 5, 4, ed, 2, None) == -1 and b"null pointer" in err()
    calls = (("dbgsom_ctx_combined_error_query", lambda c, M, E: (c, one, 0, 10, 4, w, M, ed, E, one, one)),
             ("dbgsom_ctx_combined_error_query_device", lambda c, M, E: (c, one, 0, 10, 4, 4, w, M, ed, E, one, one)),
             ("dbgsom_ctx_combined_error_query_csr", lambda c, M, E: (c, one, one, one, 0, 10, 4, 3, w, M, ed, E, one, one)))
    for name, args in calls:
        assert getattr(lib, name)(*args(None, 5, 2)) == -1 and b"null context" in err()
        with pytest.raises(ValueError, match="null context"):
            _native.call(name, *args(None, 5, 2))
        assert getattr(lib, name)(*args(ctx, 0, 2)) == -1 and b"MAX_PROTOTYPES" in err()
        assert getattr(lib, name)(*args(ctx, big, 2)) == -1 and b"MAX_PROTOTYPES" in err()
        assert getattr(lib, name)(*args(ctx, 1, 0)) == -1 and b"k <= M" in err()       # fewer than two prototypes
        assert getattr(lib, name)(*args(ctx, 5, -1)) == -1 and b"E" in err()
    assert lib.dbgsom_ctx_combined_error_query_device(ctx, one, 0, 10, 4, 3, w, 5, ed, 2, one, one) == -1 and b"ldx" in err()
