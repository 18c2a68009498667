"""Helpers of the device-level tests of the graph and label kernels (tests/test_gpu_topofn_device.py,
tests/test_topofn_device_cpu.py): crafted inputs of dbgsom_topofn, dbgsom_class_histogram_weighted and
dbgsom_topographic_weight, and plain references of the three operations.  Importable without a GPU.

dbgsom_topofn (csrc/topofn.hip): `reference` is a breadth-first search from every source over adjacency sets and
the two histograms exactly as include/dbgsom_hip.h defines them.  The generators return (idx2, xy, M) and aim at
what the BMU pairs of a fitted map never reach: histogram bins above the LDS bins (TF_HB), frontiers wider than a
workgroup, a hop distance of M - 1, a neighbour list longer than one round of the fill loop, `cols` at capacity,
M around the 32-bit word edges, n = 0, and M = DBGSOM_MAX_PROTOTYPES (more than 64 KB of LDS per workgroup)."""
import functools

import numpy as np

TF_BLOCK, TF_HB = 256, 1024          # topofn.hip: threads per workgroup, LDS bins per histogram
MAX_PROTOTYPES = 16000
RB = 1024                            # stats.hip: partial sums of topographic_w_kernel (256 threads each)


# ---- dbgsom_topofn: the reference ---------------------------------------------------------------------------------
def n_pos_of(xy):
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    return int((xy.max(axis=0) - xy.min(axis=0)).max()) + 1


def adjacency(idx2, M):
    """adjacency sets of the undirected graph of the pairs: self-pairs dropped, repeats counted once"""
    adj = [set() for _ in range(M)]
    for a, b in np.asarray(idx2, dtype=np.int64).reshape(-1, 2).tolist():
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    return adj


def lattice_pairs(xy):
    """the ordered pairs (i, j) with |dx| + |dy| == 1, by coordinate lookup"""
    pts = np.asarray(xy, dtype=np.int64).reshape(-1, 2).tolist()
    where = {(x, y): i for i, (x, y) in enumerate(pts)}
    assert len(where) == len(pts), "two neurons share coordinates"
    out = []
    for i, (x, y) in enumerate(pts):
        for p in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            j = where.get(p)
            if j is not None:
                out.append((i, j))
    return out


def reference(idx2, xy, M):
    """-> (hist_pos[n_pos], hist_neg[M + 1], D[M, M]) as int64, int64, int32 (-1 = no path)"""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    assert xy.shape[0] == M
    adj = adjacency(idx2, M)
    D = np.empty((M, M), dtype=np.int32)
    for s in range(M):
        dist = [-1] * M
        dist[s] = 0
        seen, frontier, level = {s}, {s}, 0
        while frontier:
            level += 1
            nxt = set()
            for u in frontier:
                nxt |= adj[u]
            nxt -= seen
            seen |= nxt
            for v in nxt:
                dist[v] = level
            frontier = nxt
        D[s] = dist
    hist_pos = np.zeros(n_pos_of(xy), dtype=np.int64)
    pts = xy.tolist()
    for a in range(M):
        for b in adj[a]:
            hist_pos[max(abs(pts[a][0] - pts[b][0]), abs(pts[a][1] - pts[b][1]))] += 1
    hist_neg = np.zeros(M + 1, dtype=np.int64)
    for i, j in lattice_pairs(xy):
        t = int(D[i, j])
        hist_neg[t if t >= 0 else M] += 1
    return hist_pos, hist_neg, D


# ---- dbgsom_topofn: the graphs --------------------------------------------------------------------------------------
def _pairs(p):
    return np.ascontiguousarray(np.asarray(p, dtype=np.int64).reshape(-1, 2))


def _line(M):
    return np.c_[np.arange(M), np.zeros(M, dtype=np.int64)].astype(np.int32)


def _grid(rows, cols):
    i, j = np.divmod(np.arange(rows * cols), cols)
    return np.c_[i, j].astype(np.int32)


def evens_then_odds_path(M=1500):
    """the path 0, 2, .., M - 2, M - 1, M - 3, .., 1 on the line (i, 0): hop distances up to M - 1 (the bound of the
    search's level loop), lattice neighbours 1 .. M - 1 hops apart (hist_neg's global bins)"""
    assert M % 2 == 0
    order = list(range(0, M, 2)) + list(range(M - 1, 0, -2))
    return _pairs(list(zip(order[:-1], order[1:]))), _line(M), M


LONG_RANGE_PAIRS = [(0, 1299), (1, 1100), (5, 1029), (7, 1030), (0, 1)]


def long_range_edges(M=1300):
    """edges of Chebyshev distance 1299, 1099, 1024, 1023 and 1 on the line: hist_pos on both sides of TF_HB"""
    assert M >= 1300
    return _pairs(LONG_RANGE_PAIRS), _line(M), M


def star(M=2100, hub=777):
    """the hub with every other neuron, a 42 x 50 grid in index order: a first frontier of M - 1 (more than 8
    strides of a workgroup), and a row of M - 1 neighbours in the words 0 .. 65: both rounds of the fill loop"""
    assert M == 42 * 50 and 0 <= hub < M
    others = np.delete(np.arange(M), hub)
    return _pairs(np.c_[np.full(M - 1, hub), others]), _grid(42, 50), M


HOT_PAIR = (3, 28)
HOT_OTHERS = {0: (0, 1), 17: (28, 3), 4999: (1, 2), 50_000: (39, 38), 77_777: (10, 35), 99_999: (29, 28)}


def hot_pair(n=100_000):
    """every row the same pair, a handful of others: the read before the atomicOr of the edge set"""
    idx2 = np.tile(np.array(HOT_PAIR, dtype=np.int64), (n, 1))
    for row, p in HOT_OTHERS.items():
        idx2[row] = p
    return _pairs(idx2), _grid(5, 8), 40


def _scattered(M, side, shift, rng):
    """M distinct cells of a side x side square, in random index order, shifted"""
    cells = rng.choice(side * side, M, replace=False)
    i, j = np.divmod(cells, side)
    return (np.c_[i, j] + np.asarray(shift)).astype(np.int32)


def complete(M):
    """every ordered pair once (`cols` holds M (M - 1) entries) on an irregular set with negative coordinates"""
    rng = np.random.default_rng(1000 + M)
    a, b = np.nonzero(~np.eye(M, dtype=bool))
    idx2 = np.c_[a, b][rng.permutation(a.size)]
    side = int(np.ceil(np.sqrt(2.0 * M))) + 1
    return _pairs(idx2), _scattered(M, side, (-5, -side + 2), rng), M


RANDOM_M = [1, 31, 32, 33, 64, 257, 2049]
COMPLETE_M = [2, 33, 65]


def random_components(M):
    """about 1.2 M random pairs with self-pairs and repeats among them and a few neurons left out, on a grid with
    about 15 % holes shifted to negative coordinates: several components, pairs without a path.  M = 1: n = 0."""
    rng = np.random.default_rng(4000 + M)
    side = int(np.ceil(np.sqrt(M / 0.85)))
    xy = _scattered(M, side, (-side - 1, -side - 3), rng)
    if M == 1:
        return np.zeros((0, 2), dtype=np.int64), xy, M
    isolated = rng.choice(M, max(2, M // 16), replace=False)
    live = np.setdiff1d(np.arange(M), isolated)
    n = int(1.2 * M)
    idx2 = live[rng.integers(0, live.size, (n, 2))]
    selfs = rng.choice(n, max(1, n // 20), replace=False)
    idx2[selfs, 1] = idx2[selfs, 0]
    rep = rng.choice(n, max(2, n // 10), replace=False)
    half = rep.size // 2
    idx2[rep[:half]] = idx2[rep[half:2 * half]]                  # repeats, the first quarter of them reversed
    idx2[rep[:half // 2]] = idx2[rep[:half // 2], ::-1]
    return _pairs(idx2), xy, M


def grid_edges(rows, cols):
    """the lattice's own 4-neighbour pairs of a rows x cols grid in index order, each once"""
    k = np.arange(rows * cols).reshape(rows, cols)
    return _pairs(np.r_[np.c_[k[:, :-1].ravel(), k[:, 1:].ravel()], np.c_[k[:-1].ravel(), k[1:].ravel()]])


def grid_at_limit(rows=125, cols=128):
    """M = DBGSOM_MAX_PROTOTYPES: the only shape whose search needs more than 64 KB of LDS per workgroup
    (4 ceil(M / 32) + 2 ((M + 1) & ~1) + 2 M bytes > 65536 from M = 15887 on)"""
    return grid_edges(rows, cols), _grid(rows, cols), rows * cols


def grid_closed_form(rows, cols):
    """-> (hist_pos, hist_neg) of grid_at_limit: the graph is the lattice, so D[i, j] = |di| + |dj| and every edge
    and every lattice pair lies in bin 1"""
    M = rows * cols
    hist_pos = np.zeros(max(rows, cols), dtype=np.int64)
    hist_neg = np.zeros(M + 1, dtype=np.int64)
    hist_pos[1] = hist_neg[1] = 2 * (rows * (cols - 1) + (rows - 1) * cols)
    return hist_pos, hist_neg


def grid_closed_form_D(rows, cols):
    i, j = np.divmod(np.arange(rows * cols), cols)
    return (np.abs(i[:, None] - i[None, :]) + np.abs(j[:, None] - j[None, :])).astype(np.int32)


def bfs_lds_bytes(M, full=True):
    """dynamic LDS of the search kernel, as dbgsom_topofn computes it"""
    return 4 * ((M + 31) // 32) + 2 * ((M + 1) & ~1) + (2 * M if full else 0)


# the cases whose reference is a search on the host: name -> generator call
CASES = {"path": evens_then_odds_path, "long_range": long_range_edges, "star": star, "hot_pair": hot_pair}
CASES.update({f"complete_{M}": functools.partial(complete, M) for M in COMPLETE_M})
CASES.update({f"random_{M}": functools.partial(random_components, M) for M in RANDOM_M})


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (idx2, xy, M, (hist_pos, hist_neg, D)): made once, shared by the tests, read only"""
    idx2, xy, M = CASES[name]()
    ref = reference(idx2, xy, M)
    for a in (idx2, xy) + ref:
        a.setflags(write=False)
    return idx2, xy, M, ref


def empty_graph_expected(xy, M):
    """n = 0: every lattice pair without a path, no edge, D = 0 on the diagonal and -1 elsewhere"""
    hist_pos = np.zeros(n_pos_of(xy), dtype=np.int64)
    hist_neg = np.zeros(M + 1, dtype=np.int64)
    hist_neg[M] = len(lattice_pairs(xy))
    D = np.full((M, M), -1, dtype=np.int32)
    np.fill_diagonal(D, 0)
    return hist_pos, hist_neg, D


# ---- dbgsom_class_histogram_weighted --------------------------------------------------------------------------------
# (N, M, C): C > 256 takes the per-thread class loop (nc = ceil(C / 256)), lists longer than 256 rows several tiles
# (a list of 600 rows and one of 256 do not fit into 700 rows: (700, 5, 7) has 400 and 256, (900, 5, 7) has 600 and 256)
CLASS_SHAPES = [(0, 3, 4), (1, 1, 1), (700, 5, 7), (900, 5, 7), (900, 4, 256), (900, 4, 257), (1500, 3, 600)]
CLASS_COUNTS = {(700, 5, 7): [400, 0, 256, 43, 1],          # several tiles, an empty list, exactly one tile
                (900, 5, 7): [600, 0, 256, 43, 1]}


def bucket(winners, M):
    """-> (order int32, seg_start uint32 with M + 1 entries): the rows bucketed by winner, stable"""
    winners = np.asarray(winners, dtype=np.int64)
    order = np.argsort(winners, kind="stable").astype(np.int32)
    seg_start = np.zeros(M + 1, dtype=np.uint32)
    seg_start[1:] = np.cumsum(np.bincount(winners, minlength=M))
    return order, seg_start


def class_inputs(N, M, C, integer_weights=False):
    """-> (winners int64, y int32 with a few labels at -1 and >= C, w float64 with zeros)"""
    rng = np.random.default_rng(N + 7 * M + 13 * C)
    counts = CLASS_COUNTS.get((N, M, C))
    if counts is None:
        winners = rng.integers(0, M, N).astype(np.int64)
    else:
        assert sum(counts) == N and len(counts) == M
        winners = np.repeat(np.arange(M, dtype=np.int64), counts)[rng.permutation(N)]
    y = rng.integers(0, C, N).astype(np.int32)
    if N:
        y[-1] = C - 1                                             # the last class of the last round is met
    bad = rng.choice(N, N // 40, replace=False)
    y[bad[::2]], y[bad[1::2]] = -1, C + rng.integers(0, 3, bad[1::2].size).astype(np.int32)
    if integer_weights:
        w = rng.integers(0, 6, N).astype(np.float64)
    else:
        w = rng.uniform(0.05, 3.0, N)
        w[rng.random(N) < 0.1] = 0.0
    return winners, y, w


def class_hist_loop(order, seg_start, y, w, n, M, C):
    """the float64 weights added one after the other in list order, every list clamped at n"""
    hist = np.zeros((M, C), dtype=np.float64)
    for j in range(M):
        for p in range(int(seg_start[j]), min(int(seg_start[j + 1]), n)):
            r = int(order[p])
            if 0 <= y[r] < C:
                hist[j, y[r]] = hist[j, y[r]] + w[r]
    return hist


# ---- dbgsom_topographic_weight ------------------------------------------------------------------------------------
TOPO_N = [0, 1, 257, 300_000]        # the last one: more than RB * 256 rows, a thread takes a second row
TOPO_ROWS, TOPO_COLS, TOPO_SHIFT = 5, 6, (-7, -11)


def topo_inputs(n, weights="frac"):
    """-> (idx2 with some pairs at -1 or M, w, xy of a 5 x 6 lattice at negative coordinates, M)"""
    rng = np.random.default_rng(n + 3)
    M = TOPO_ROWS * TOPO_COLS
    xy = (_grid(TOPO_ROWS, TOPO_COLS) + np.asarray(TOPO_SHIFT)).astype(np.int32)
    idx2 = rng.integers(0, M, (n, 2)).astype(np.int64)
    near = rng.random(n) < 0.5                                   # half the rows: second BMU one step away
    step = np.array([1, -1, TOPO_COLS, -TOPO_COLS, TOPO_COLS + 1, 2])[rng.integers(0, 6, n)]
    idx2[near, 1] = np.clip(idx2[near, 0] + step[near], 0, M - 1)
    bad = rng.choice(n, n // 50, replace=False)
    idx2[bad[::2], rng.integers(0, 2, bad[::2].size)] = -1
    idx2[bad[1::2], rng.integers(0, 2, bad[1::2].size)] = M
    if weights == "frac":
        w = rng.uniform(0.0, 3.0, n)
        w[rng.random(n) < 0.1] = 0.0
    elif weights == "int":
        w = rng.integers(0, 5, n).astype(np.float64)
    else:
        w = np.ones(n, dtype=np.float64)
    return _pairs(idx2), w, xy, M


def topo_counted(idx2, xy, M):
    """the rows dbgsom_topographic_count counts: both indices inside [0, M), lattice positions further than 1.5
    apart (squared distance > 2.25, in integers: >= 3)"""
    a, b = idx2[:, 0], idx2[:, 1]
    ok = (a >= 0) & (a < M) & (b >= 0) & (b < M)
    p = np.asarray(xy, dtype=np.int64)
    d = p[np.where(ok, a, 0)] - p[np.where(ok, b, 0)]
    return ok & ((d * d).sum(axis=1) >= 3)
