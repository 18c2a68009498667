"""MI355X: dbgsom_topofn (csrc/topofn.hip), dbgsom_class_histogram_weighted and dbgsom_topographic_weight
(csrc/stats.hip) called raw through include/dbgsom_hip.h on crafted inputs (tests/topofn_device.py) that the BMU
pairs of a fitted map and the context's label histograms never produce: histogram bins above the LDS bins, search
frontiers wider than a workgroup, a hop distance of M - 1, a neighbour list of two fill rounds, `cols` at capacity,
M = 1, 2 and around the 32-bit word edges, n = 0, M = DBGSOM_MAX_PROTOTYPES (more than 64 KB of LDS), the three
status results; more than 256 classes, lists of several tiles, lists clamped at n; a second row per thread.

Histograms, hop distances, integer-weight sums and the list-order float64 sums are compared bit for bit with plain
host references, the summed weight within n u sum |w_i| of the exact rational sum.  Outputs, the elements behind
them and the workspace are pre-filled with non-zero bytes."""
import ctypes
import time
from fractions import Fraction

import numpy as np
import pytest

from tests import device_abi as da
from tests import topofn_device as td

pytestmark = pytest.mark.gpu
GUARD = 64                              # elements behind an output that must stay as they were
HIST_FILL, D_FILL = 0x5A5A5A5A5A5A5A5A, -77
OK, EINVAL, ERANGE = 0, -1, -5


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


def _sync():
    import torch

    torch.cuda.synchronize()


def _full(shape, value, dtype):
    import torch

    return torch.full(shape, value, dtype=getattr(torch, dtype), device="cuda")


def _dev(a):
    """a device copy; an empty array travels as one element (a valid pointer), the call's n says it is empty"""
    a = np.ascontiguousarray(a)
    return da.dev(a if a.size else np.zeros(1, dtype=a.dtype))


# ---- dbgsom_topofn ------------------------------------------------------------------------------------------------
class Graph:
    """the device inputs of one graph and a workspace full of non-zero bytes"""

    def __init__(self, nat, idx2, xy, M, n_pos=None):
        self.lib = nat.load()
        self.n, self.M = len(idx2), M
        self.n_pos = td.n_pos_of(xy) if n_pos is None else n_pos
        self.idx2 = da.dev(np.array(idx2)) if len(idx2) else None          # (copies: the shared cases are read only)
        self.xy = da.dev(np.array(xy, dtype=np.int32))
        self.nbytes = self.lib.dbgsom_topofn_workspace_bytes(M, 1)
        assert self.nbytes > 0 and self.nbytes == self.lib.dbgsom_topofn_workspace_bytes(M, 0)
        self.ws_t, self.ws = da.workspace(self.nbytes)
        self.ws_t.fill_(0xA5)

    def run(self, full, idx2=None, xy=None, n_pos=None):
        """-> (status, hist_pos, hist_neg, D or None) as device tensors with their guards"""
        n_pos = self.n_pos if n_pos is None else n_pos
        idx2 = self.idx2 if idx2 is None else idx2
        hp = _full((n_pos + GUARD,), HIST_FILL, "int64")
        hn = _full((self.M + 1 + GUARD,), HIST_FILL, "int64")
        D = _full((self.M * self.M + GUARD,), D_FILL, "int32") if full else None
        rc = self.lib.dbgsom_topofn(None if idx2 is None else idx2.data_ptr(), self.n, (self.xy if xy is None else xy).data_ptr(),
                                    self.M, n_pos, hp.data_ptr(), hn.data_ptr(), None if D is None else D.data_ptr(),
                                    self.ws, self.nbytes, da.stream())
        _sync()
        return rc, hp, hn, D

    def results(self, full, **kw):
        """a call that must succeed -> (hist_pos, hist_neg, D or None) on the host, the guards checked"""
        rc, hp, hn, D = self.run(full, **kw)
        assert rc == OK, self.lib.dbgsom_last_error()
        n_pos = kw.get("n_pos") or self.n_pos
        hp, hn = hp.cpu().numpy(), hn.cpu().numpy()
        assert (hp[n_pos:] == HIST_FILL).all() and (hn[self.M + 1:] == HIST_FILL).all()
        if D is not None:
            D = D.cpu().numpy()
            assert (D[self.M * self.M:] == D_FILL).all()
            D = D[:self.M * self.M].reshape(self.M, self.M)
        return hp[:n_pos], hn[:self.M + 1], D


def _check_all_modes(g, want):
    wp, wn, WD = want
    hp, hn, D = g.results(full=True)
    assert np.array_equal(D, WD)
    assert np.array_equal(hp, wp) and np.array_equal(hn, wn)
    hp2, hn2, D2 = g.results(full=True)                      # the workspace now holds the first call's leftovers
    assert np.array_equal(hp2, hp) and np.array_equal(hn2, hn) and np.array_equal(D2, D)
    hp3, hn3, none = g.results(full=False)
    assert none is None and np.array_equal(hp3, hp) and np.array_equal(hn3, hn)
    hp4, hn4, _ = g.results(full=False)
    assert np.array_equal(hp4, hp) and np.array_equal(hn4, hn)


@pytest.mark.parametrize("name", list(td.CASES))
def test_topofn_equals_the_breadth_first_reference(nat, name):
    idx2, xy, M, want = td.case(name)
    _check_all_modes(Graph(nat, idx2, xy, M), want)


def test_topofn_without_pairs(nat):
    xy = td._grid(5, 8)
    want = td.empty_graph_expected(xy, 40)
    assert want[1][40] == 134 and want[2].sum() == -(40 * 39)
    _check_all_modes(Graph(nat, np.zeros((0, 2), dtype=np.int64), xy, 40), want)


def test_topofn_at_the_prototype_limit(nat):
    """M = DBGSOM_MAX_PROTOTYPES on a 125 x 128 grid whose edges are the lattice's own: the only shape at which the
    search kernel asks for more than 64 KB of LDS.  D is compared on the device with its closed form.
    Measured on an MI355X: 0.38 s for the whole test (the full-mode call 11.9 ms, the histogram-mode call 3.1 ms),
    beside 0.17 s of test_histogram_mode_equals_full_mode_at_8000 in the same run."""
    import torch

    rows, cols = 125, 128
    idx2, xy, M = td.grid_at_limit(rows, cols)
    assert M == td.MAX_PROTOTYPES and td.bfs_lds_bytes(M) > 65536
    wp, wn = td.grid_closed_form(rows, cols)
    g = Graph(nat, idx2, xy, M)
    _sync()
    t0 = time.perf_counter()
    rc, hp, hn, D = g.run(full=True)
    t_full = time.perf_counter() - t0
    assert rc == OK, g.lib.dbgsom_last_error()
    assert np.array_equal(hp.cpu().numpy()[:cols], wp) and np.array_equal(hn.cpu().numpy()[:M + 1], wn)
    assert (hp[cols:] == HIST_FILL).all() and (hn[M + 1:] == HIST_FILL).all() and (D[M * M:] == D_FILL).all()
    k = torch.arange(M, device="cuda", dtype=torch.int32)
    ki, kj = k // cols, k % cols
    step = 2000
    for r0 in range(0, M, step):
        want = (ki[r0:r0 + step, None] - ki[None, :]).abs() + (kj[r0:r0 + step, None] - kj[None, :]).abs()
        assert torch.equal(D[r0 * M:(r0 + step) * M].view(step, M), want), f"rows {r0} .. {r0 + step}"
    del D, want
    t0 = time.perf_counter()
    hp2, hn2, none = g.results(full=False)
    t_hist = time.perf_counter() - t0
    print(f"dbgsom_topofn at M = {M}: full mode {t_full * 1e3:.1f} ms, histogram mode {t_hist * 1e3:.1f} ms")
    assert none is None and np.array_equal(hp2, wp) and np.array_equal(hn2, wn)


def _status_graph(nat):
    """a 5 x 8 grid with its own edges and one edge across the whole width (Chebyshev distance 7 = n_pos - 1)"""
    xy = td._grid(5, 8)
    idx2 = np.r_[td.grid_edges(5, 8), [[0, 7]], [[12, 12]]]
    g = Graph(nat, idx2, xy, 40)
    want = td.reference(idx2, xy, 40)
    assert g.n_pos == 8 and want[0][7] == 2
    return g, idx2, xy, want


def _failed(g, rc, code, what):
    msg = g.lib.dbgsom_last_error()
    assert rc == code and b"dbgsom_topofn" in msg and what in msg, (rc, msg)


@pytest.mark.parametrize("bad", [-1, 40])
@pytest.mark.parametrize("full", [True, False])
def test_topofn_reports_an_index_outside_the_map(nat, full, bad):
    """-1 is what a k = 2 search returns for a row without any value"""
    g, idx2, xy, want = _status_graph(nat)
    for row, col in ((0, 0), (len(idx2) - 1, 1)):
        wrong = idx2.copy()
        wrong[row, col] = bad
        rc = g.run(full, idx2=da.dev(wrong))[0]
        _failed(g, rc, ERANGE, b"outside [0, 40)")
        _check_all_modes(g, want)                             # the status word is reset


def test_topofn_reports_an_edge_longer_than_n_pos(nat):
    g, idx2, xy, want = _status_graph(nat)
    for full in (True, False):
        rc, hp, hn, D = g.run(full, n_pos=7)
        _failed(g, rc, EINVAL, b">= n_pos = 7")
        assert (hp[7:] == HIST_FILL).all()                    # nothing written behind the n_pos bins
        _check_all_modes(g, want)
    wider = g.results(full=True, n_pos=9)                     # a larger n_pos is no error: one more empty bin
    assert np.array_equal(wider[0], np.r_[want[0], 0]) and np.array_equal(wider[1], want[1])


def test_topofn_reports_shared_coordinates(nat):
    g, idx2, xy, want = _status_graph(nat)
    for i, j in ((5, 6), (39, 0)):
        twice = xy.copy()
        twice[i] = twice[j]
        for full in (True, False):
            rc = g.run(full, xy=da.dev(twice))[0]
            _failed(g, rc, EINVAL, b"share lattice coordinates")
        _check_all_modes(g, want)


def test_topofn_stage_timing(nat):
    lib = nat.load()
    idx2, xy, M, want = td.case("random_257")
    g = Graph(nat, idx2, xy, M)
    ms = (ctypes.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    try:
        assert lib.dbgsom_topofn_timing(1) == OK
        hp, hn, D = g.results(full=True)
        assert lib.dbgsom_topofn_stage_ms(ms) == OK
        assert ms[0] == 0.0 and all(ms[i] > 0.0 for i in (1, 2, 3)), list(ms)       # a raw call makes no search
        assert np.array_equal(hp, want[0]) and np.array_equal(hn, want[1]) and np.array_equal(D, want[2])
    finally:
        assert lib.dbgsom_topofn_timing(0) == OK
    assert lib.dbgsom_topofn_stage_ms(ms) == OK and list(ms) == [0.0, 0.0, 0.0, 0.0]
    g.results(full=False)
    assert lib.dbgsom_topofn_stage_ms(ms) == OK and list(ms) == [0.0, 0.0, 0.0, 0.0]   # off: nothing is summed


# ---- dbgsom_class_histogram_weighted --------------------------------------------------------------------------------
def _class_hist_w(nat, order, seg, y, w, n, M, C):
    """-> M x C float64 on the host; NaN in front, the guard behind checked"""
    keep = [_dev(order), da.dev(seg), _dev(y), _dev(w)]
    hist = _full((M * C + GUARD,), float("nan"), "float64")
    nat.call("dbgsom_class_histogram_weighted", *(t.data_ptr() for t in keep), n, M, C, hist.data_ptr(), da.stream())
    _sync()
    got = hist.cpu().numpy()
    assert np.isnan(got[M * C:]).all()
    return got[:M * C].reshape(M, C)


def _class_counts(nat, winners, y, n, M, C):
    keep = [_dev(winners), _dev(y)]
    hist = _full((M * C,), -1, "int64")
    nat.call("dbgsom_class_histogram", *(t.data_ptr() for t in keep), n, M, C, hist.data_ptr(), da.stream())
    _sync()
    return hist.cpu().numpy().reshape(M, C)


@pytest.mark.parametrize("N,M,C", td.CLASS_SHAPES)
def test_class_histogram_weighted_adds_in_list_order(nat, N, M, C):
    winners, y, w = td.class_inputs(N, M, C)
    order, seg = td.bucket(winners, M)
    got = _class_hist_w(nat, order, seg, y, w, N, M, C)
    assert np.array_equal(got, td.class_hist_loop(order, seg, y, w, N, M, C))
    if N >= 2:                                                # n below seg_start[M]: every list ends at n
        for n in (N // 2, int(seg[1]) if 0 < seg[1] < N else 1):
            got = _class_hist_w(nat, order, seg, y, w, n, M, C)
            assert np.array_equal(got, td.class_hist_loop(order, seg, y, w, n, M, C))


@pytest.mark.parametrize("N,M,C", td.CLASS_SHAPES)
def test_class_histogram_weighted_with_integer_weights_is_exact(nat, N, M, C):
    winners, y, w = td.class_inputs(N, M, C, integer_weights=True)
    order, seg = td.bucket(winners, M)
    ok = (y >= 0) & (y < C)
    want = np.zeros((M, C))
    np.add.at(want, (winners[ok], y[ok]), w[ok])
    assert np.array_equal(_class_hist_w(nat, order, seg, y, w, N, M, C), want)
    counts = _class_counts(nat, winners, y, N, M, C)
    assert np.array_equal(counts, np.bincount(winners[ok] * C + y[ok], minlength=M * C).reshape(M, C))
    got = _class_hist_w(nat, order, seg, y, np.full(N, 3.0), N, M, C)
    assert np.array_equal(got, 3.0 * counts)


# ---- dbgsom_topographic_weight ------------------------------------------------------------------------------------
def _topo_weight(nat, idx2_t, w_t, n, xy_t, M, ws, nbytes):
    out = _full((1 + GUARD,), float("nan"), "float64")
    nat.call("dbgsom_topographic_weight", idx2_t.data_ptr(), w_t.data_ptr(), n, xy_t.data_ptr(), M, out.data_ptr(),
             ws, nbytes, da.stream())
    _sync()
    got = out.cpu().numpy()
    assert np.isnan(got[1:]).all()
    return got[:1]


@pytest.mark.parametrize("n", td.TOPO_N)
def test_topographic_weight(nat, n):
    """|got - exact| <= n u sum |w_i| over the counted rows, against their exact (rational) sum; the same bits on
    a second call; exact with integer weights; dbgsom_topographic_count with weights of one"""
    lib = nat.load()
    nbytes = lib.dbgsom_sum_workspace_bytes()
    ws_t, ws = da.workspace(nbytes)
    ws_t.fill_(0xA5)
    idx2, w, xy, M = td.topo_inputs(n, "frac")
    counted = td.topo_counted(idx2, xy, M)
    idx2_t, xy_t = _dev(idx2), da.dev(xy)
    got = [_topo_weight(nat, idx2_t, _dev(w), n, xy_t, M, ws, nbytes) for _ in range(2)]
    assert np.array_equal(got[0], got[1])
    exact, T = da.exact_sum(w[counted])
    err = abs(Fraction(float(got[0][0])) - exact)
    bound = n * Fraction(da.U) * T
    print(f"dbgsom_topographic_weight n = {n}: error / bound {float(err / bound) if bound else float(err):.3f}")
    assert err <= bound
    w_int = td.topo_inputs(n, "int")[1]
    assert _topo_weight(nat, idx2_t, _dev(w_int), n, xy_t, M, ws, nbytes)[0] == w_int[counted].sum()
    count = _full((1,), -1, "int64")
    nat.call("dbgsom_topographic_count", idx2_t.data_ptr(), n, xy_t.data_ptr(), M, count.data_ptr(), da.stream())
    _sync()
    assert int(count.cpu()[0]) == int(counted.sum())
    assert _topo_weight(nat, idx2_t, _dev(np.ones(n)), n, xy_t, M, ws, nbytes)[0] == float(counted.sum())
