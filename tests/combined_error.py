"""Helpers of the combined-error tests (tests/test_combined_error_cpu.py, tests/test_gpu_combined_error.py): the NumPy
restatement of csrc/geodesics.hip, the table of graphs the geodesic kernel is run on, and a CPU stand-in backend.

The contract (include/dbgsom_hip.h).
  len(a, b) = sqrt(s), s = 0 and then, k ascending, t = W[a, k] - W[b, k], p = t * t, s = s + p, every operation rounded
  on its own in float64.
  G[s, t] = the minimum over lattice paths s = v0, .., vn = t of the left fold ((0 + len(v0, v1)) + len(v1, v2)) + ...;
  G[s, s] = 0, +inf without a path.  Rounded addition of a non-negative length is monotone, so that minimum is the least
  fixed point of dist[v] = min(dist[v], dist[u] + len(u, v)) from dist[s] = 0: Bellman-Ford rounds here, Dijkstra in
  scipy and the chaotic relaxation of the kernel end in the same bits.
  e_i = d1_i + G[b1_i, b2_i] on the first and second result of the search at k = 2 without float32 rounding; NaN for a
  row with -1 in either slot."""
import functools

import numpy as np

from oracle import som_oracle as o
from tests import device_abi as da
from tests import distortion as ds
from tests import prototype_distances as pd

U = 2.0 ** -53
SENTINEL = pd.SENTINEL
NT_SMALL, NT_LARGE = 256, 1024       # lanes of a workgroup of geodesic_kernel: the stride over the edge list
LDS_SMALL_M = 8192                   # the largest M whose vector fits 64 KiB of LDS (and runs with NT_SMALL lanes)
MAX_M = 16000


# ---- the restatement ------------------------------------------------------------------------------------------------
def edge_lengths(W, edges):
    """W: M x d float64, edges: E x 2 -> E float64"""
    W = np.ascontiguousarray(W, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    s = np.zeros(len(edges))
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(W.shape[1]):
            t = W[edges[:, 0], k] - W[edges[:, 1], k]
            p = t * t
            s = s + p
        return np.sqrt(s)


def directed(edges, lengths):
    """both directions of every edge that is no self-loop -> (u, v, l)"""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    lengths = np.asarray(lengths, dtype=np.float64)
    keep = edges[:, 0] != edges[:, 1]
    a, b, l = edges[keep, 0], edges[keep, 1], lengths[keep]
    return np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([l, l])


def geodesics(M, edges, lengths, sources=None, want_rounds=False):
    """Bellman-Ford in synchronous rounds (every candidate of a round is formed on the vector the round began with),
    all sources at once -> G (S x M); with want_rounds also the number of rounds that lowered something."""
    sources = np.arange(M) if sources is None else np.asarray(sources, dtype=np.int64)
    u, v, l = directed(edges, lengths)
    dist = np.full((len(sources), M), np.inf)
    dist[np.arange(len(sources)), sources] = 0.0
    rounds = 0
    if len(u):
        order = np.argsort(v, kind="stable")
        u, v, l = u[order], v[order], l[order]
        heads, starts = np.unique(v, return_index=True)
        for _ in range(max(M - 1, 1)):
            cand = np.minimum.reduceat(dist[:, u] + l[None, :], starts, axis=1)
            new = np.minimum(dist[:, heads], cand)
            if np.array_equal(new, dist[:, heads]):
                break
            dist[:, heads] = new
            rounds += 1
    return (dist, rounds) if want_rounds else dist


def two_nearest(X, W):
    """(d2, idx2) of the oracle's chain search at k = 2, float64 prototypes: no float32 rounding"""
    Xw = np.ascontiguousarray(da.widen(np.asarray(X)))
    return o.bmu_chain(Xw, np.ascontiguousarray(W, dtype=np.float64), 2)


def combined_error_rows(idx2, d1, G):
    """e = d1 + G[b1, b2]; NaN where either index is -1"""
    idx2 = np.asarray(idx2, dtype=np.int64)
    ok = (idx2 >= 0).all(axis=1)
    e = np.full(len(idx2), np.nan)
    e[ok] = np.asarray(d1, dtype=np.float64)[ok] + G[idx2[ok, 0], idx2[ok, 1]]
    return e


def combined_error(X, W, edges):
    """-> (e, idx2) of complete rows"""
    W = np.ascontiguousarray(W, dtype=np.float64)
    d2, idx2 = two_nearest(X, W)
    G = geodesics(len(W), edges, edge_lengths(W, edges))
    return combined_error_rows(idx2, d2[:, 0], G), idx2


# ---- the graph table ------------------------------------------------------------------------------------------------
def lattice_edges(rows, cols):
    n = np.arange(rows * cols).reshape(rows, cols)
    right = np.stack([n[:, :-1].ravel(), n[:, 1:].ravel()], axis=1)
    down = np.stack([n[:-1].ravel(), n[1:].ravel()], axis=1)
    return np.concatenate([right, down]).astype(np.int32)


def path_edges(n_edges):
    i = np.arange(n_edges, dtype=np.int32)
    return np.stack([i, i + 1], axis=1)


def _lengths(n, seed):
    return np.random.default_rng(seed).random(n) + 0.125


def _single():
    return 1, np.empty((0, 2), np.int32), np.empty(0), None


def _pair():
    return 2, np.array([[1, 0]], np.int32), np.array([1.5]), None


def _path300():
    return 300, path_edges(299), _lengths(299, 1), None


def _holes16():
    """a 16 x 16 sheet whose units 34, 35, 100 and 255 lost their edges, cut in two between rows 9 and 10; the lengths
    are those of random prototypes (d = 3)"""
    edges = lattice_edges(16, 16)
    gone = np.isin(edges, [34, 35, 100, 255]).any(axis=1) | ((edges[:, 0] // 16 == 9) & (edges[:, 1] // 16 == 10))
    edges = edges[~gone]
    W = np.random.default_rng(16).normal(size=(256, 3))
    return 256, edges, edge_lengths(W, edges), None


def _star():
    leaves = np.arange(1, 2100, dtype=np.int32)
    return 2100, np.stack([np.zeros_like(leaves), leaves], axis=1), _lengths(2099, 2), None


def _cycle200():
    i = np.arange(200, dtype=np.int32)
    lengths = np.ones(200)
    lengths[199] = 1e6                       # the edge (199, 0)
    return 200, np.stack([i, (i + 1) % 200], axis=1), lengths, None


def _duplicates():
    """a 5 x 6 sheet whose prototypes 7 and 8 (neighbours) are equal: a zero-length edge"""
    W = np.random.default_rng(5).normal(size=(30, 4))
    W[8] = W[7]
    edges = lattice_edges(5, 6)
    return 30, edges, edge_lengths(W, edges), None


def _loops_and_repeats():
    edges = np.array([[0, 1], [1, 1], [1, 2], [2, 1], [0, 1], [2, 3], [3, 3], [3, 4], [0, 4], [1, 0], [4, 5], [5, 5]], np.int32)
    lengths = np.array([3.0, 0.5, 1.0, 0.75, 2.0, 1.0, 0.0, 1.0, 9.0, 2.5, 1.0, 7.0])
    return 6, edges, lengths, None


def _inf_edge():
    lengths = _lengths(9, 3)
    lengths[4] = np.inf                      # 0 .. 4 and 5 .. 9 stay apart
    return 10, path_edges(9), lengths, None


def _wide_range():
    return 31, path_edges(30), 10.0 ** np.linspace(-150, 150, 30), None


def _stride(n_edges, M):
    """a path of n_edges edges through the first n_edges + 1 of M units (the others stay alone)"""
    def make():
        sources = None if M <= 300 else np.array([0, n_edges // 2, n_edges, M - 1], np.int32)
        return M, path_edges(n_edges), _lengths(n_edges, n_edges), sources
    return make


def _sheet(rows, cols, extra, sources):
    """a rows x cols sheet and `extra` units behind it, the first of them hanging on the last unit of the sheet"""
    def make():
        edges = lattice_edges(rows, cols)
        if extra:
            edges = np.concatenate([edges, np.array([[rows * cols - 1, rows * cols]], np.int32)])
        return rows * cols + extra, edges, _lengths(len(edges), rows), np.asarray(sources, np.int32)
    return make


GRAPHS = {
    "single": _single,                       # M = 1, no edge
    "pair": _pair,                           # M = 2, one edge
    "path300": _path300,                     # 299 rounds from either end
    "holes16": _holes16,                     # holes and several components
    "star": _star,                           # degree 2099
    "cycle200": _cycle200,                   # 199 hops where breadth-first depth is 1
    "duplicates": _duplicates,               # a zero-length edge
    "loops_and_repeats": _loops_and_repeats,
    "inf_edge": _inf_edge,
    "wide_range": _wide_range,               # 1e-150 .. 1e150 on one path
    "stride255": _stride(NT_SMALL - 1, NT_SMALL),          # E at both ends of a small workgroup's stride, one past it
    "stride256": _stride(NT_SMALL, NT_SMALL + 1),
    "stride257": _stride(NT_SMALL + 1, NT_SMALL + 2),
    "stride1023": _stride(NT_LARGE - 1, LDS_SMALL_M + 8),  # ... and of a large one's
    "stride1024": _stride(NT_LARGE, LDS_SMALL_M + 8),
    "stride1025": _stride(NT_LARGE + 1, LDS_SMALL_M + 8),
    "lds64k": _sheet(64, 128, 0, [0, 4100, 8191]),         # M = 8192: the last that fits 64 KiB of LDS
    "lds64k+1": _sheet(64, 128, 1, [0, 4100, 8192]),       # M = 8193: the first that does not
    "max": _sheet(125, 128, 0, [0, 8000, 15999]),          # M = 16000: first, middle and last source
}
GRAPH_IDS = list(GRAPHS)


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (M, edges, lengths, sources or None, G): a table entry and the restatement's rows, computed once and shared
    (read only)"""
    M, edges, lengths, sources = GRAPHS[name]()
    G = geodesics(M, edges, lengths, sources)
    for a in (edges, lengths, sources, G):
        if a is not None:
            a.setflags(write=False)
    return M, edges, lengths, sources, G


def scipy_rows(M, edges, lengths, sources):
    """scipy's Dijkstra on the same graph: self-loops and +inf edges left out, of repeated edges the shortest"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    u, v, l = directed(edges, lengths)
    best = {}
    for a, b, w in zip(u.tolist(), v.tolist(), l.tolist()):
        if w < np.inf and w < best.get((a, b), np.inf):
            best[(a, b)] = w
    if best:
        rc = np.array(list(best), dtype=np.int64)
        A = csr_matrix((np.array(list(best.values())), (rc[:, 0], rc[:, 1])), shape=(M, M))
    else:
        A = csr_matrix((M, M))
    return dijkstra(A, directed=True, indices=None if sources is None else np.asarray(sources))


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------
class CombinedErrorOracleBackend(ds.DistortionOracleBackend):
    """DistortionOracleBackend with ``geodesics`` / ``combined_error`` from the restatement (TESTS ONLY); records the
    rows and the edges of every call."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.combined_rows, self.combined_edges = [], []

    def geodesics(self, W, edges):
        W = np.ascontiguousarray(W, dtype=np.float64)
        return geodesics(len(W), edges, edge_lengths(W, edges))

    def combined_error(self, W, edges, X):
        if hasattr(X, "toarray"):
            X = X.toarray()
        X = np.ascontiguousarray(X)
        assert not np.isnan(X).any()
        self.combined_rows.append(len(X))
        self.combined_edges.append(np.array(edges))
        return combined_error(X, W, edges)
