"""MI355X: candidate lists from the anchors (csrc/filter.hip 2f) at device level -- dbgsom_anchor_runs_build and
dbgsom_bmu_filtered_anchor_runs called raw, what they leave behind read back (dbgsom_anchor_runs_read,
dbgsom_bmu_filtered_anchor_bounds, dbgsom_bmu_filtered_lists) and held against tests/anchor_mark.py:

* the run table: run_start and the anchors are NumPy's; R is an upper bound of the largest exact distance of the run and
  within the stated margin (d + 8) 2^-52 of it, XXmax is the largest of the norms the call was given;
* low[a][j] <= |a - w_j|^2 and up[a] >= |a - w_seed(a)| against np.longdouble, and neither is vacuous;
* the lists hold every prototype within 2 rho_i of a sample's nearest (the all-pairs arg-min set and more);
* winners and distances are dbgsom_bmu's bits (and oracle.som_oracle.bmu_chain's on the table of shapes).

N in {300, 1000, 4096} x d in {16, 70, 320} x M in {130, 256} x storage f32 / f64 / bf16 (d = 70 padded to 80 with
zeros, as the context pads; bf16: the table from the stored rows, the search on their float32 copy), then the special
inputs and a map whose lists come out long, which the per-sample pass must take over."""
import numpy as np
import pytest

from tests import anchor_mark as am
from tests import device_abi as da
from tests import test_gpu_filter_device as tfd

pytestmark = pytest.mark.gpu

PRUNE, PRUNE_RETRY = 0x200, 0x800
L = np.longdouble


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


def _pad(A, dp):
    out = np.zeros((A.shape[0], dp), dtype=A.dtype)
    out[:, :A.shape[1]] = A
    return out


def _values(X, storage):
    """-> (what is stored, the float32 / float64 rows the search reads), padded to whole 16 features"""
    dp = (X.shape[1] + 15) // 16 * 16
    if storage == "f64":
        X = X.astype(np.float64) * (1.0 + 2.0 ** -30)          # (float64 rows that are no float32 values)
    st = da.stored(_pad(np.asarray(X), dp), storage)
    return st, np.ascontiguousarray(da.widen(st))


def run_case(nat, o, X, W, storage, A=256, flags=PRUNE, buckets=None):
    """one table build and one search -> everything read back, and the inputs as the device saw them"""
    import torch

    st, Xs = _values(X, storage)                               # Xs: float32 (f32, bf16) or float64
    N, dp = Xs.shape
    M = W.shape[0]
    Wp = _pad(np.asarray(W, dtype=np.float64), dp)
    anchors, aof, order = buckets(Xs) if buckets else am.buckets(Xs, A)
    A = anchors.shape[0]
    search = "f64" if storage == "f64" else "f32"
    xt, xptr = da.stage(Xs, dp, 0, search)
    stt, stptr = (xt, xptr) if storage != "bf16" else da.stage(st, dp, 0, "bf16")
    Mg = (M + 63) // 64 * 64
    wt = torch.zeros((Mg, dp), dtype=torch.float64, device="cuda")
    wt[:M] = da.dev(Wp)
    xx = tfd._norms(nat, xptr, da.CODE[search], N, dp, dp)
    ww = torch.zeros((Mg,), dtype=torch.float64, device="cuda")
    ww[:M] = tfd._norms(nat, wt.data_ptr(), da.F64, M, dp, dp)
    lib = nat.load()
    pbytes = lib.dbgsom_filter_planes_bytes(N, dp)
    pt, pptr = tfd._filled(pbytes, 0x7f)
    nat.call("dbgsom_filter_prepare", xptr, da.CODE[search], N, dp, dp, pptr, pbytes, da.stream())
    a_t, of_t, or_t = da.dev(anchors), da.dev(aof), da.dev(order)
    rbytes = lib.dbgsom_anchor_runs_bytes(N, A)
    assert rbytes > 256
    rt, rptr = tfd._filled(rbytes, 0x7f)                       # (not zeroed: the builder owes nothing to the allocator)
    nat.call("dbgsom_anchor_runs_build", stptr, da.CODE[storage], N, dp, dp, xx.data_ptr(), a_t.data_ptr(), A,
             of_t.data_ptr(), or_t.data_ptr(), rptr, rbytes, da.stream())
    nb = (N + 127) // 128
    cap = nb + A
    start = np.full(nb + 1, -7, dtype=np.int32)
    ranchor, rR, rxx = np.full(cap, -7, dtype=np.int32), np.full(cap, np.nan), np.full(cap, np.nan)
    nat.call("dbgsom_anchor_runs_read", rptr, N, A, start.ctypes.data, ranchor.ctypes.data, rR.ctypes.data, rxx.ctypes.data,
             da.stream())
    assert (tfd._bytes_at(rt, rptr, rbytes + 256)[rbytes:] == 0x7f).all(), "dbgsom_anchor_runs_build wrote behind its table"
    wbytes = tfd._workspace_bytes(nat, N, dp, M)
    ws_t, ws = da.workspace(wbytes)
    idx, dist = tfd._full((N,), -7, "int64"), tfd._full((N,), float("nan"), "float64")
    nat.call("dbgsom_bmu_filtered_anchor_runs", xptr, da.CODE[search], N, dp, dp, xx.data_ptr(), pptr, wt.data_ptr(), M,
             ww.data_ptr(), a_t.data_ptr(), A, of_t.data_ptr(), or_t.data_ptr(), rptr, flags, 0, 0, idx.data_ptr(),
             dist.data_ptr(), ws, wbytes, da.stream())
    tfd._sync()
    ref_idx, ref_dist = tfd._full((N,), -7, "int64"), tfd._full((N,), float("nan"), "float64")
    nat.call("dbgsom_bmu", xptr, da.CODE[search], N, dp, dp, xx.data_ptr(), wt.data_ptr(), M, ww.data_ptr(), 1, 0,
             ref_idx.data_ptr(), ref_dist.data_ptr(), da.stream())
    tfd._sync()
    counts = np.full(nb, 0xffffffff, dtype=np.uint32)
    nat.call("dbgsom_bmu_filtered_counts", ws, N, dp, M, counts.ctypes.data, nb, da.stream())
    lists = np.full((nb, M), 0xffff, dtype=np.uint16)
    nat.call("dbgsom_bmu_filtered_lists", ws, N, dp, M, lists.ctypes.data, da.stream())
    low, up, c2 = np.full((A, M), np.nan, dtype=np.float32), np.full(A, np.nan), np.zeros(2, dtype=np.uint64)
    nat.call("dbgsom_bmu_filtered_anchor_bounds", ws, N, dp, M, A, low.ctypes.data, up.ctypes.data, c2.ctypes.data, da.stream())
    aseed = np.full(A, -7, dtype=np.int32)
    nat.call("dbgsom_bmu_filtered_anchor_seeds", ws, N, dp, M, A, aseed.ctypes.data, None, da.stream())
    n = int(start[-1])
    del xt, stt, wt, pt, rt, a_t, of_t, or_t
    return {"Xs": Xs, "Wp": Wp, "anchors": anchors, "aof": aof, "order": order, "xx": xx.cpu().numpy(), "run_start": start,
            "anchor": ranchor[:n], "R": rR[:n], "xx_max": rxx[:n], "idx": idx.cpu().numpy(), "dist": dist.cpu().numpy(),
            "counts": counts.astype(np.int64), "lists": lists, "low": low, "up": up, "handed": int(c2[0]),
            "still_long": int(c2[1]), "aseed": aseed,
            "ref_idx": ref_idx.cpu().numpy(), "ref_dist": ref_dist.cpu().numpy(), "tickets_zero": not tfd._bytes_at(ws_t, ws, 256).any()}


def check_table(got):
    Xs, dp = got["Xs"], got["Xs"].shape[1]
    ref = am.run_table(Xs, got["anchors"], got["aof"], got["order"], xx=got["xx"])
    assert np.array_equal(got["run_start"], ref["run_start"])
    assert np.array_equal(got["anchor"], ref["anchor"])
    lo, hi = am.widened_R(ref["R2"], dp)
    fin = np.isfinite(ref["R2"].astype(np.float64))
    assert (got["R"][fin].astype(L) >= lo[fin]).all(), "R is not an upper bound"
    assert (got["R"][fin].astype(L) <= hi[fin]).all(), "R beyond the stated margin"
    assert np.isposinf(got["R"][~fin]).all() and np.isposinf(got["xx_max"][~fin]).all()
    assert np.array_equal(got["xx_max"][fin], ref["xx_max"][fin])          # (the largest of the norms the call brought)
    # ... which are |x_i|^2 themselves to the rounding of a float64 sum
    xl = (Xs.astype(np.float64).astype(L) ** 2).sum(axis=1).astype(np.float64)
    ok = np.isfinite(xl)
    assert np.allclose(got["xx"][ok], xl[ok], rtol=(dp + 2) * 2.0 ** -52, atol=0)
    return ref


def check_bounds(got):
    a, Wp = got["anchors"], got["Wp"]
    A, dp = a.shape
    fin_w, fin_a = am.finite_rows(Wp), am.finite_rows(a)
    with np.errstate(over="ignore", invalid="ignore"):
        r = am.exact_r(np.where(fin_a[:, None], a, 0.0), np.where(fin_w[:, None], Wp, 0.0))
        aa, ww = (a * a).sum(axis=1), (Wp * Wp).sum(axis=1)
    low = got["low"].astype(L)
    both = fin_a[:, None] & fin_w[None, :]
    assert (low[both] <= r[both]).all(), "low is not a lower bound of |a - w_j|^2"
    assert not got["low"][~both].any(), "a bound for a row or an anchor that is not finite"
    if np.isfinite(ww[fin_w]).all() and np.isfinite(ww).all():
        # not vacuous: within the cancellation margin (2 rho_a) and float32's rounding of the exact value
        rho_a = 4.0 * (dp + 16) * am.U * (aa + ww.max())
        floor = r * L(1.0 - 2.0 ** -22) - (2.0 * rho_a[:, None]).astype(L)
        big = both & (floor > 1e-30)
        assert (low[big] >= floor[big]).all(), "low is far below |a - w_j|^2"
        rs = r[np.arange(A), got["aseed"]]
        ok = fin_a & fin_w[got["aseed"]]
        with np.errstate(invalid="ignore"):
            assert (got["up"][ok].astype(L) >= np.sqrt(np.maximum(rs[ok], 0))).all(), "up is not an upper bound"
            assert (got["up"][ok].astype(L) <= np.sqrt(np.maximum(rs[ok], 0) + (2.0 * rho_a[ok]).astype(L)) * L(1 + 1e-9)).all()
        assert np.isposinf(got["up"][~fin_a]).all()


def check_lists(got, slack=0.01):
    keep = am.must_keep(got["Xs"], got["Wp"], slack=slack)
    need = am.group_sets(keep, got["order"])
    M = got["Wp"].shape[0]
    for g, must in enumerate(need):
        n = got["counts"][g]
        assert 1 <= n <= M, (g, n)
        have = got["lists"][g, :n].astype(np.int64)
        assert (np.diff(have) > 0).all() and have[-1] < M
        missing = np.setdiff1d(must, have)
        assert missing.size == 0, (g, missing[:8])


def check_exact(o, got, oracle=False):
    """winners and distances: dbgsom_bmu's bits on the same device arrays (and, on finite inputs, the oracle's)"""
    assert np.array_equal(got["idx"], got["ref_idx"]), int((got["idx"] != got["ref_idx"]).sum())
    assert np.array_equal(got["dist"], got["ref_dist"], equal_nan=True), int((got["dist"] != got["ref_dist"]).sum())
    fin = np.isfinite(got["xx"])      # (a row with a NaN has no winner: whatever dbgsom_bmu answers, the same here)
    assert (got["ref_idx"][fin] >= 0).all() and (got["ref_idx"][fin] < got["Wp"].shape[0]).all()
    if oracle:
        rd, ri = o.bmu_chain(got["Xs"], got["Wp"], 1)
        assert np.array_equal(got["idx"], ri) and np.array_equal(got["dist"], rd)
    assert got["tickets_zero"]


# ---- 1. the table of shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("N,d,M", [(N, d, M) for N in (300, 1000, 4096) for d in (16, 70, 320) for M in (130, 256)])
def test_shapes(nat, o, N, d, M, storage):
    X, W = am.blobs(N, d, M, "device")
    got = run_case(nat, o, X, W, storage)
    check_table(got)
    check_bounds(got)
    check_lists(got)
    check_exact(o, got, oracle=True)
    print(f"N={N} d={d} M={M} {storage}: {len(got['anchor'])} runs, mean list {got['counts'].mean():.1f}, "
          f"{got['handed']} of {len(got['counts'])} workgroups handed to the per-sample pass, {got['still_long']} still long")
    assert got["handed"] <= len(got["counts"]) and got["still_long"] <= got["handed"]


# ---- 2. special inputs ------------------------------------------------------------------------------------------------
def test_fewer_rows_than_anchors_every_row_its_own_anchor(nat, o):
    X, W = am.blobs(200, 48, 130, "small")
    got = run_case(nat, o, X, W, "f32")
    ref = check_table(got)
    assert len(got["anchor"]) == 200 and got["run_start"][1] == 128 and not got["R"].any()
    assert np.array_equal(got["anchor"], np.arange(200))
    check_bounds(got), check_lists(got), check_exact(o, got)


def test_rows_no_multiple_of_the_workgroup_and_one_sample_in_the_last(nat, o):
    X, W = am.blobs(129 + 256, 32, 130, "tail")
    got = run_case(nat, o, X, W, "f64", A=16)
    check_table(got), check_bounds(got), check_lists(got), check_exact(o, got)
    assert got["run_start"][-1] - got["run_start"][-2] == 1


def test_a_workgroup_spanning_many_anchors(nat, o):
    """256 anchors over 1000 rows: four rows per bucket, some thirty runs per workgroup"""
    X, W = am.blobs(1000, 32, 256, "span")
    got = run_case(nat, o, X, W, "f32", A=256)
    check_table(got), check_bounds(got), check_lists(got), check_exact(o, got)
    per = np.diff(got["run_start"])
    assert per.max() >= 3 and per.max() > 8, per


@pytest.mark.parametrize("bad", ["nan_prototype", "inf_prototype", "nan_sample", "nan_anchor"])
def test_rows_that_are_not_finite(nat, o, bad):
    X, W = am.blobs(1000, 32, 130, "bad")
    if bad == "nan_prototype":
        W[5, 3] = np.nan
    elif bad == "inf_prototype":
        W[5, 3] = np.inf
    elif bad == "nan_sample":
        X[501, 7] = np.nan                       # (no anchor row: 1000 k / 64 is never 501)
    else:
        X[500, 7] = np.nan                       # (anchor row 32 of 64)
    got = run_case(nat, o, X, W, "f32", A=64)
    ref = check_table(got)
    check_bounds(got), check_lists(got), check_exact(o, got)
    M = 130
    if bad == "nan_prototype":                   # no bound for it: in every list; the other bounds stand
        assert all(5 in got["lists"][g, :n] for g, n in enumerate(got["counts"])) and got["counts"].min() < M
        assert (got["aseed"] != 5).all()
    elif bad == "inf_prototype":                 # max |w|^2 is infinite: no margin, no bound, the whole map everywhere
        assert (got["counts"] == M).all() and got["handed"] == len(got["counts"])
    else:
        row = 501 if bad == "nan_sample" else 500
        g = int(np.flatnonzero(got["order"] == row)[0]) // 128
        assert got["counts"][g] == M and got["counts"].min() < M
        assert np.isposinf(got["R"]).sum() >= 1


def test_every_row_identical(nat, o):
    rng = am.rng_for("identical")
    X = np.tile(rng.standard_normal((1, 48)).astype(np.float32), (600, 1))
    W = rng.standard_normal((130, 48))
    got = run_case(nat, o, X, W, "f32")
    check_table(got), check_bounds(got), check_lists(got), check_exact(o, got)
    assert not got["R"].any()


def test_buckets_in_no_order_overflow_the_table_and_take_the_whole_map(nat, o):
    """a bucket order that is not sorted by anchor has more runs than the table holds: workgroups whose runs did not
    fit take every prototype (and the per-sample pass behind them prunes as ever)"""
    X, W = am.blobs(4096, 16, 130, "shuffled")

    def shuffled(Xs):
        anchors, aof, order = am.buckets(Xs, 16)
        return anchors, aof, am.rng_for("perm").permutation(len(order)).astype(np.int32)

    got = run_case(nat, o, X, W, "f32", buckets=shuffled)
    check_lists(got), check_exact(o, got)
    assert got["run_start"][-1] > 32 + 16 and got["handed"] >= 1


# ---- 3. lists that come out long go to the per-sample pass ------------------------------------------------------------
@pytest.mark.parametrize("flags", [PRUNE, PRUNE | PRUNE_RETRY], ids=["plain", "retry"])
def test_long_lists_are_handed_to_the_per_sample_pass(nat, o, flags):
    """clusters 2.5 radii apart: twice the bucket radius rules little out from the anchor, the sample's own distance
    to its seed rules out more.  Measured on MI355X: all 32 workgroups handed over; behind the per-sample pass the
    mean list is 253.4 of 256, 215.3 with the re-seeding passes -- every one still long: such data is the sweep's."""
    X, W = am.blobs(4096, 70, 256, "close", radii=2.5)
    got = run_case(nat, o, X, W, "f32", flags=flags)
    check_table(got), check_bounds(got), check_lists(got), check_exact(o, got)
    print(f"handed {got['handed']} of {len(got['counts'])}, still long {got['still_long']}, mean list {got['counts'].mean():.1f}")
    assert got["handed"] > 0, "no workgroup exceeded the threshold: the case does not reach the per-sample pass"
    assert got["still_long"] <= got["handed"]
    # what anchor_mark_kernel alone would have left those workgroups, from the table and the bounds read back
    _, _, _, yy_max = am.bounds(got["anchors"], got["Wp"])
    table = {"run_start": got["run_start"], "anchor": got["anchor"], "xx_max": got["xx_max"]}
    alone = am.rule_lists(got["R"], table, got["low"], got["up"], got["aseed"], yy_max, 256, got["Xs"].shape[1])
    n_long = sum(len(h) > am.long_above(256) for h in alone)
    assert n_long == got["handed"], (n_long, got["handed"])
    for g, h in enumerate(alone):
        if len(h) <= am.long_above(256):
            assert np.array_equal(got["lists"][g, :got["counts"][g]], h), g
