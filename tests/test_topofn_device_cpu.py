"""CPU: the helpers of the device-level tests of the graph and label kernels (tests/topofn_device.py) do what they
say -- the plain breadth-first reference agrees with scipy's unweighted shortest paths and with the histogram
stage of HotPathBackend.topographic_function, every crafted graph has the property it was made for -- and the
argument errors of dbgsom_topofn, dbgsom_topographic_weight and dbgsom_class_histogram_weighted that return before
any HIP call come back as status codes with a message."""
import os

import numpy as np
import pytest

from tests import topofn_device as td

EINVAL, ENOMEM = -1, -3


@pytest.fixture(scope="module")
def lib():
    from dbgsom_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.load()


class _Pairs:
    """stands in for a backend: the k = 2 search of the host default returns the given pairs"""

    def __init__(self, idx2):
        self.idx2 = idx2

    def bmu(self, W, k, X=None):
        assert k == 2
        return None, self.idx2


def host_default(idx2, xy):
    """HotPathBackend.topographic_function from the pairs on: scipy's shortest_path(unweighted=True) and the
    histogram code of the host default"""
    from dbgsom_amd.backend import HotPathBackend

    return HotPathBackend.topographic_function(_Pairs(idx2), None, None, xy, want_distances=True)


# ---- the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in td.CASES if k != "random_1"])
def test_reference_equals_scipy_and_the_host_default(name):
    idx2, xy, M, (hp, hn, D) = td.case(name)
    assert M <= 2100 and idx2.dtype == np.int64 and xy.dtype == np.int32 and xy.shape == (M, 2)
    assert hp.shape == (td.n_pos_of(xy),) and hn.shape == (M + 1,) and D.shape == (M, M) and D.dtype == np.int32
    rp, rn, RD = host_default(idx2, xy)
    assert np.array_equal(D, RD)
    assert np.array_equal(hp, rp) and np.array_equal(hn, rn)


def test_reference_on_a_hand_made_graph():
    """0 - 1 - 2 and 3 alone on a 2 x 2 square: [[0, 0], [0, 1], [1, 0], [1, 1]]; a self-pair and a repeat"""
    idx2 = np.array([[0, 1], [1, 2], [2, 2], [1, 0], [0, 1]])
    hp, hn, D = td.reference(idx2, td._grid(2, 2), 4)
    assert D.tolist() == [[0, 1, 2, -1], [1, 0, 1, -1], [2, 1, 0, -1], [-1, -1, -1, 0]]
    assert hp.tolist() == [0, 4]                    # 0-1 and 1-2 both ways, Chebyshev distance 1 (1-2 is a diagonal)
    # lattice pairs: 0-1 (1 hop), 0-2 (2 hops), 1-3 and 2-3 (no path), both ways
    assert hn.tolist() == [0, 2, 2, 0, 4]


# ---- the graphs ---------------------------------------------------------------------------------------------------
def test_path_reaches_the_last_level_and_the_global_bins_of_hist_neg():
    idx2, xy, M, (hp, hn, D) = td.case("path")
    assert M == 1500 and D.max() == M - 1 and D.min() == 0
    assert hn[td.TF_HB:M].sum() == 952 and hn[M] == 0
    assert np.flatnonzero(hp).tolist() == [1, 2] and hp[1] == 2 and hp[2] == 2996


def test_long_range_edges_straddle_the_lds_bins_of_hist_pos():
    idx2, xy, M, (hp, hn, D) = td.case("long_range")
    assert M == 1300 and np.flatnonzero(hp).tolist() == [1, 1023, 1024, 1099, 1299] and (hp[hp > 0] == 2).all()
    assert 1023 < td.TF_HB <= 1024
    assert hn[M] == 2596 and hn[1] == 2 and hn.sum() == 2598


def test_star_has_a_wide_frontier_and_a_row_of_two_fill_rounds():
    idx2, xy, M, (hp, hn, D) = td.case("star")
    adj = td.adjacency(idx2, M)
    assert len(adj[777]) == 2099 > 8 * td.TF_BLOCK
    assert sorted({v >> 5 for v in adj[777]}) == list(range(66))          # words 0 .. 65: more than one round of 64
    assert min(adj[777]) < 2048 < max(adj[777])
    assert D.max() == 2
    assert np.flatnonzero(hn).tolist() == [1, 2] and hn[1] == 8 and hn[2] == 8208


def test_hot_pair_equals_its_deduplicated_pairs():
    idx2, xy, M, ref = td.case("hot_pair")
    assert idx2.shape == (100_000, 2) and M == 40
    assert (idx2 == np.array(td.HOT_PAIR)).all(axis=1).sum() == 100_000 - len(td.HOT_OTHERS)
    uniq = np.unique(idx2, axis=0)
    assert len(uniq) == 1 + len(td.HOT_OTHERS)
    for a, b in zip(ref, td.reference(uniq, xy, M)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("M", td.COMPLETE_M)
def test_complete_fills_cols(M):
    idx2, xy, M_, (hp, hn, D) = td.case(f"complete_{M}")
    assert M_ == M and len(idx2) == M * (M - 1) and len(np.unique(idx2, axis=0)) == M * (M - 1)
    assert sum(len(a) for a in td.adjacency(idx2, M)) == M * (M - 1)
    assert xy.min() < 0 and len(np.unique(xy, axis=0)) == M
    assert (D[~np.eye(M, dtype=bool)] == 1).all() and hp.sum() == M * (M - 1)


@pytest.mark.parametrize("M", td.RANDOM_M)
def test_random_components_have_pairs_without_a_path(M):
    idx2, xy, M_, (hp, hn, D) = td.case(f"random_{M}")
    assert M_ == M and xy.max() < 0 and len(np.unique(xy, axis=0)) == M
    if M == 1:
        assert idx2.shape == (0, 2) and D.tolist() == [[0]] and hn.tolist() == [0, 0] and hp.tolist() == [0]
        return
    assert len(idx2) == int(1.2 * M)
    assert (idx2[:, 0] == idx2[:, 1]).any()                                         # self-pairs
    assert len(np.unique(np.sort(idx2, axis=1), axis=0)) < len(idx2)                # repeats
    assert any(not a for a in td.adjacency(idx2, M))                                # isolated neurons
    side = int(np.ceil(np.sqrt(M / 0.85)))
    assert M <= 0.87 * side * side                                                  # holes
    assert hn[M] > 0 and (D < 0).any() and hn[1:M].sum() > 0 and hp.sum() > 0


def test_grid_at_limit_closed_forms():
    idx2, xy, M = td.grid_at_limit(5, 8)
    hp, hn, D = td.reference(idx2, xy, M)
    cp, cn = td.grid_closed_form(5, 8)
    assert np.array_equal(hp, cp) and np.array_equal(hn, cn) and np.array_equal(D, td.grid_closed_form_D(5, 8))
    assert cp[1] == 2 * (5 * 7 + 4 * 8)
    idx2, xy, M = td.grid_at_limit()
    assert M == td.MAX_PROTOTYPES and len(idx2) == 125 * 127 + 124 * 128 and td.n_pos_of(xy) == 128
    assert td.grid_closed_form(125, 128)[0][1] == 2 * (125 * 127 + 124 * 128)
    # the only case above the 64 KB a workgroup has without asking: from M = 15887 on
    assert td.bfs_lds_bytes(15886) <= 65536 < td.bfs_lds_bytes(15887) <= td.bfs_lds_bytes(M) == 66000
    assert all(td.bfs_lds_bytes(td.case(k)[2]) < 65536 for k in td.CASES)


def test_empty_graph_expected():
    hp, hn, D = td.empty_graph_expected(td._grid(5, 8), 40)
    assert hp.tolist() == [0] * 8 and hn[40] == 2 * (5 * 7 + 4 * 8) and hn[:40].sum() == 0
    for a, b in zip((hp, hn, D), td.reference(np.zeros((0, 2), dtype=np.int64), td._grid(5, 8), 40)):
        assert np.array_equal(a, b)


# ---- the inputs of the two stats calls --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,C", td.CLASS_SHAPES)
def test_class_inputs_and_the_list_order_loop(N, M, C):
    winners, y, w = td.class_inputs(N, M, C)
    order, seg = td.bucket(winners, M)
    assert order.dtype == np.int32 and seg.dtype == np.uint32 and seg.shape == (M + 1,) and seg[M] == N
    for j in range(M):
        rows = order[seg[j]:seg[j + 1]]
        assert (winners[rows] == j).all() and (np.diff(rows) > 0).all()             # stable: ascending row ids
    if N >= 700:
        assert (y == -1).any() and (y >= C).any() and (w == 0).any() and (w != np.round(w)).any()
        assert (y == C - 1).any()
    if (N, M, C) in td.CLASS_COUNTS:
        assert np.diff(seg.astype(np.int64)).tolist() == [N - 300, 0, 256, 43, 1]
    hist = td.class_hist_loop(order, seg, y, w, N, M, C)
    ok = (y >= 0) & (y < C)
    want = np.zeros((M, C))
    np.add.at(want, (winners[ok], y[ok]), w[ok])
    np.testing.assert_allclose(hist, want, rtol=1e-12, atol=0)
    # integer weights: every order of adding gives the same bits
    winners, y, w = td.class_inputs(N, M, C, integer_weights=True)
    order, seg = td.bucket(winners, M)
    ok = (y >= 0) & (y < C)
    want = np.zeros((M, C))
    np.add.at(want, (winners[ok], y[ok]), w[ok])
    assert np.array_equal(td.class_hist_loop(order, seg, y, w, N, M, C), want)
    # clamped at n: the rows behind position n of the bucket order do not count
    n = N // 2
    head = order[:n]
    ok = (y[head] >= 0) & (y[head] < C)
    want = np.zeros((M, C))
    np.add.at(want, (winners[head][ok], y[head][ok]), w[head][ok])
    assert np.array_equal(td.class_hist_loop(order, seg, y, w, n, M, C), want)


@pytest.mark.parametrize("n", td.TOPO_N)
def test_topo_inputs(n):
    idx2, w, xy, M = td.topo_inputs(n)
    assert M == 30 and xy.max() < 0 and idx2.shape == (n, 2)
    counted = td.topo_counted(idx2, xy, M)
    if n >= 257:
        assert (idx2 == -1).any() and (idx2 == M).any() and counted.any() and not counted.all()
        ok = ((idx2 >= 0) & (idx2 < M)).all(axis=1)
        d = xy[idx2[ok, 0]].astype(np.float64) - xy[idx2[ok, 1]]
        dist = np.sqrt((d * d).sum(axis=1))
        assert np.array_equal(counted[ok], dist > 1.5)
        assert ((dist > 1.0) & (dist <= 1.5)).any()                  # diagonal steps: the threshold is what decides
    assert n <= td.RB * 256 or n == 300_000


# ---- argument errors that return before any HIP call ----------------------------------------------------------------
P = 0x10000          # a fake, 256-byte aligned device address: never dereferenced on these paths


def _topofn(lib, *, idx2=P, n=10, xy=P, M=5, n_pos=3, hp=P, hn=P, D=None, ws=P, ws_bytes=None):
    need = lib.dbgsom_topofn_workspace_bytes(min(max(M, 1), td.MAX_PROTOTYPES), int(D is not None))
    return lib.dbgsom_topofn(idx2, n, xy, M, n_pos, hp, hn, D, ws, need if ws_bytes is None else ws_bytes, None)


def test_argument_errors_of_topofn(lib):
    def failed(rc, code, what):
        msg = lib.dbgsom_last_error()
        assert rc == code and b"dbgsom_topofn" in msg and what in msg, (rc, msg)

    failed(_topofn(lib, M=0), EINVAL, b"DBGSOM_MAX_PROTOTYPES")
    failed(_topofn(lib, M=td.MAX_PROTOTYPES + 1), EINVAL, b"DBGSOM_MAX_PROTOTYPES")
    failed(_topofn(lib, n=-1), EINVAL, b"bad shape")
    failed(_topofn(lib, n_pos=0), EINVAL, b"bad shape")
    failed(_topofn(lib, xy=None), EINVAL, b"null pointer")
    failed(_topofn(lib, hp=None), EINVAL, b"null pointer")
    failed(_topofn(lib, hn=None), EINVAL, b"null pointer")
    failed(_topofn(lib, idx2=None, n=1), EINVAL, b"null pointer")
    failed(_topofn(lib, ws=None), EINVAL, b"null pointer")
    for D in (None, P):
        need = lib.dbgsom_topofn_workspace_bytes(5, int(D is not None))
        failed(_topofn(lib, D=D, ws_bytes=need - 1), ENOMEM, b"workspace too small")
        failed(_topofn(lib, D=D, ws=P + 4), EINVAL, b"256-byte aligned")
        failed(_topofn(lib, D=D, ws=P + 128), EINVAL, b"256-byte aligned")


def test_topofn_workspace_bytes(lib):
    for full in (0, 1):
        assert lib.dbgsom_topofn_workspace_bytes(0, full) == 0
        assert lib.dbgsom_topofn_workspace_bytes(-1, full) == 0
        assert lib.dbgsom_topofn_workspace_bytes(td.MAX_PROTOTYPES + 1, full) == 0
    for M in (1, 2, 33, 2100, td.MAX_PROTOTYPES):
        need = lib.dbgsom_topofn_workspace_bytes(M, 0)
        assert need == lib.dbgsom_topofn_workspace_bytes(M, 1) and need % 256 == 0
        # status word, bitmap, row offsets, two M x 4 tables, every ordered pair as a uint16 column
        assert need >= 4 + 4 * M * ((M + 31) // 32) + 4 * (M + 1) + 32 * M + 2 * M * (M - 1)


def test_argument_errors_of_the_weighted_stats_calls(lib):
    def failed(rc, code, what):
        msg = lib.dbgsom_last_error()
        assert rc == code and what in msg, (rc, msg)

    need = 8 * td.RB

    def weight(idx2=P, w=P, n=10, xy=P, M=5, out=P, ws=P, ws_bytes=need):
        return lib.dbgsom_topographic_weight(idx2, w, n, xy, M, out, ws, ws_bytes, None)

    failed(weight(n=-1), EINVAL, b"dbgsom_topographic_weight: bad arguments")
    failed(weight(M=0), EINVAL, b"bad arguments")
    failed(weight(M=2 ** 31), EINVAL, b"bad arguments")
    failed(weight(out=None), EINVAL, b"bad arguments")
    failed(weight(ws=None), EINVAL, b"bad arguments")
    failed(weight(idx2=None), EINVAL, b"dbgsom_topographic_weight: null pointer")
    failed(weight(w=None), EINVAL, b"null pointer")
    failed(weight(xy=None), EINVAL, b"null pointer")
    failed(weight(ws_bytes=need - 1), ENOMEM, b"dbgsom_topographic_weight: workspace too small")
    failed(weight(n=0, idx2=None, w=None, xy=None, ws_bytes=need - 1), ENOMEM, b"workspace too small")

    def hist(order=P, seg=P, y=P, w=P, n=10, M=5, C=3, out=P):
        return lib.dbgsom_class_histogram_weighted(order, seg, y, w, n, M, C, out, None)

    failed(hist(n=-1), EINVAL, b"dbgsom_class_histogram_weighted: bad arguments")
    failed(hist(M=0), EINVAL, b"bad arguments")
    failed(hist(M=2 ** 31), EINVAL, b"bad arguments")
    failed(hist(C=0), EINVAL, b"bad arguments")
    failed(hist(C=2 ** 31), EINVAL, b"bad arguments")
    failed(hist(out=None), EINVAL, b"bad arguments")
    failed(hist(order=None), EINVAL, b"dbgsom_class_histogram_weighted: null pointer")
    failed(hist(seg=None), EINVAL, b"null pointer")
    failed(hist(y=None), EINVAL, b"null pointer")
    failed(hist(w=None), EINVAL, b"null pointer")
