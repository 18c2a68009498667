"""MI355X: the lean form of the anchor-marked search at device level -- dbgsom_bmu_filtered_anchor_runs called raw with
DBGSOM_ANCHOR_LISTS_ONLY -- and anchor_seed_kernel at the edges of its split of k over the four wavefronts.

1. Lean raw calls on rows of tests/anchor_seeds.SEED_ROWS, each with the run table of its buckets: winners and distances
   are oracle.som_oracle.bmu_chain's bits; the anchors' seeds are those of the call without the bit; so are the lists
   of every workgroup whose list is not long (the call without the bit hands the long ones to the per-sample pass, the
   lean call keeps them and counts them the same); tickets at zero; the same bits from a fresh workspace and from one
   shared by every case, a full call in front of every lean one, forward and reversed.
2. What the lean form skips did not run: in a workspace filled with a byte pattern (all but the tickets, which are
   zero between launches) the plane region of W, the gap table and the per-sample seeds still hold the pattern.
3. The seed kernel at d = 16 (one k-step: three wavefronts idle), 48 (fewer steps than wavefronts) and 208 (13 steps,
   4 / 3 / 3 / 3): the arg-min by tests/anchor_seeds.check_argmin, the kept bounds against np.longdouble as
   tests/test_gpu_anchor_mark_device.py holds them, winners and distances dbgsom_bmu's bits."""
import numpy as np
import pytest

from tests import anchor_mark as am
from tests import anchor_seeds as an
from tests import device_abi as da
from tests import test_gpu_anchor_mark_device as tamd
from tests import test_gpu_anchor_seed_device as tasd
from tests import test_gpu_filter_device as tfd

pytestmark = pytest.mark.gpu

PRUNE, LISTS_ONLY = 0x200, 0x2000
PATTERN = 0x5a


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


# rows of the table with a map beyond one block of partial minima, few and many anchors, every kind of bucket, both
# types, the 129-row sample set -- and the largest map, in front of which the smaller ones run in the shared workspace
ROWS = tuple(r for r in an.SEED_ROWS if r[1] == PRUNE and r[2] in (
    (17, 130, 16, "blobs", "f64", "nearest"),
    (256, 130, 320, "iso", "f32", "random"),
    (255, 1985, 48, "iso", "f64", "nearest"),
    (256, 64, 64, "blobs", "f64", "zeros"),
    (16, 8192, 16, "blobs", "f32", "last"),
    (17, 65, 48, "blobs", "f32", "nearest"),
))
assert len(ROWS) == 6 and ROWS[4][2][1] == 8192 and ROWS[5][0] == 129      # (the last row: 129 samples)


class _Staged:
    """per row: inputs, the oracle's answer, the staged device copies and the run table of the buckets, built once"""

    def __init__(self, nat, o):
        self.nat, self.o, self.rows = nat, o, {}

    def get(self, row):
        if row not in self.rows:
            nat = self.nat
            inp = an.seed_inputs(row)
            rd, ri = self.o.bmu_chain(inp["X"], inp["W"], 1)
            st = tasd._stage(nat, inp)
            N, d, A = st["N"], st["d"], inp["anchors"].shape[0]
            dev = (da.dev(inp["anchors"]), da.dev(inp["anchor_of"].astype(np.int32)), da.dev(inp["order"].astype(np.int32)))
            rbytes = nat.load().dbgsom_anchor_runs_bytes(N, A)
            rt, rptr = tfd._filled(rbytes, 0x7f)
            nat.call("dbgsom_anchor_runs_build", st["x"], st["code"], N, d, d, st["xx"], dev[0].data_ptr(), A, dev[1].data_ptr(),
                     dev[2].data_ptr(), rptr, rbytes, da.stream())
            tfd._sync()
            self.rows[row] = (inp, st, rd, ri, dev, (rt, rptr))
        return self.rows[row]

    def call(self, row, flags, ws_t, ws, ws_bytes):
        """one dbgsom_bmu_filtered_anchor_runs call -> what it left"""
        nat = self.nat
        inp, st, _, _, dev, (_, rptr) = self.get(row)
        N, d, M, A = st["N"], st["d"], st["M"], inp["anchors"].shape[0]
        nb = (N + 127) // 128
        idx, dist = tfd._full((N,), -7, "int64"), tfd._full((N,), float("nan"), "float64")
        nat.call("dbgsom_bmu_filtered_anchor_runs", st["x"], st["code"], N, d, d, st["xx"], st["planes"], st["W"], M, st["ww"],
                 dev[0].data_ptr(), A, dev[1].data_ptr(), dev[2].data_ptr(), rptr, flags, 0, 0, idx.data_ptr(), dist.data_ptr(),
                 ws, ws_bytes, da.stream())
        tfd._sync()
        out = {"idx": idx.cpu().numpy(), "dist": dist.cpu().numpy(), "tickets_zero": not tfd._bytes_at(ws_t, ws, 256).any()}
        counts = np.full(nb, 0xffffffff, dtype=np.uint32)
        nat.call("dbgsom_bmu_filtered_counts", ws, N, d, M, counts.ctypes.data, nb, da.stream())
        lists = np.full((nb, M), 0xffff, dtype=np.uint16)
        nat.call("dbgsom_bmu_filtered_lists", ws, N, d, M, lists.ctypes.data, da.stream())
        aseed, seed = np.full(A, -7, dtype=np.int32), np.full(N, -7, dtype=np.int64)
        nat.call("dbgsom_bmu_filtered_anchor_seeds", ws, N, d, M, A, aseed.ctypes.data, seed.ctypes.data, da.stream())
        low, up, c2 = np.full((A, M), np.nan, dtype=np.float32), np.full(A, np.nan), np.zeros(2, dtype=np.uint64)
        nat.call("dbgsom_bmu_filtered_anchor_bounds", ws, N, d, M, A, low.ctypes.data, up.ctypes.data, c2.ctypes.data, da.stream())
        out.update(counts=counts.astype(np.int64), lists=lists, aseed=aseed, seed=seed, low=low, up=up, handed=int(c2[0]),
                   still_long=int(c2[1]))
        return out


@pytest.fixture(scope="module")
def staged(nat, o):
    return _Staged(nat, o)


def _ws_bytes(nat, row):
    N, _, (A, M, d, *_rest) = row
    return tfd._workspace_bytes(nat, N, d, M)


@pytest.fixture(scope="module")
def shared_runs(nat, staged):
    """every row in ONE workspace sized for the largest and zero-filled once, a full call and then the lean call per row:
    table order (the largest map's full call runs in front of the last row's lean one), then reversed"""
    sizes = [_ws_bytes(nat, r) for r in ROWS]
    ws_t, ws = da.workspace(max(sizes))
    runs = {}
    for tag, seq in (("forward", range(len(ROWS))), ("reverse", range(len(ROWS) - 1, -1, -1))):
        for ri in seq:
            staged.call(ROWS[ri], PRUNE, ws_t, ws, sizes[ri])
            runs[(tag, ri)] = staged.call(ROWS[ri], PRUNE | LISTS_ONLY, ws_t, ws, sizes[ri])
    return runs


@pytest.mark.parametrize("ri", range(len(ROWS)), ids=[an.seed_row_id(r) for r in ROWS])
def test_lean_raw_calls(nat, staged, shared_runs, ri):
    row = ROWS[ri]
    N, _, (A, M, d, *_rest) = row
    inp, _, rd, rix, _, _ = staged.get(row)
    nbytes = _ws_bytes(nat, row)
    ws_t, ws = da.workspace(nbytes)
    full = staged.call(row, PRUNE, ws_t, ws, nbytes)
    ws2_t, ws2 = da.workspace(nbytes)
    lean = staged.call(row, PRUNE | LISTS_ONLY, ws2_t, ws2, nbytes)
    assert np.array_equal(full["idx"], rix) and np.array_equal(full["dist"], rd)
    assert an.check_argmin(lean["aseed"], inp["anchors"], inp["W"]) == A
    assert np.array_equal(lean["aseed"], full["aseed"])
    assert np.array_equal(lean["low"], full["low"]) and np.array_equal(lean["up"], full["up"])   # (max |w|^2: the same bits)
    assert np.array_equal(full["seed"], full["aseed"][inp["anchor_of"]].astype(np.int64))
    assert not lean["seed"].any(), "the lean call gathered per-sample seeds (fresh workspace: zeros)"
    # the lists: the same wherever anchor_mark_kernel's list is not long; long ones are kept and counted, not handed on
    short = lean["counts"] <= am.long_above(M)
    assert int((~short).sum()) == lean["handed"] == full["handed"]
    assert lean["still_long"] == 0
    assert np.array_equal(lean["counts"][short], full["counts"][short])
    for g in np.flatnonzero(short):
        assert np.array_equal(lean["lists"][g, :lean["counts"][g]], full["lists"][g, :full["counts"][g]]), g
    for g in np.flatnonzero(~short):     # a kept list: ascending ids below M that hold every winner of the workgroup
        kept = lean["lists"][g, :lean["counts"][g]].astype(np.int64)
        assert (np.diff(kept) > 0).all() and kept[-1] < M, g
        assert np.isin(rix[inp["order"][128 * g:128 * g + 128]], kept).all(), g
    print(f"{an.seed_row_id(row)}: mean list {lean['counts'].mean():.1f} lean / {full['counts'].mean():.1f} full, "
          f"{lean['handed']} of {len(short)} workgroups long")
    for tag, got in (("fresh", lean), ("forward", shared_runs[("forward", ri)]), ("reverse", shared_runs[("reverse", ri)])):
        assert np.array_equal(got["idx"], rix), (tag, int((got["idx"] != rix).sum()))
        assert np.array_equal(got["dist"], rd), (tag, int((got["dist"] != rd).sum()))
        assert got["tickets_zero"], tag
        assert np.array_equal(got["aseed"], lean["aseed"]), (tag, "the seeds depend on what the workspace held")
        assert np.array_equal(got["counts"], lean["counts"]) and got["handed"] == lean["handed"], tag
        for g in range(len(short)):
            assert np.array_equal(got["lists"][g, :got["counts"][g]], lean["lists"][g, :lean["counts"][g]]), (tag, g)


@pytest.mark.parametrize("ri", [1, 2], ids=[an.seed_row_id(ROWS[1]), an.seed_row_id(ROWS[2])])
def test_the_skipped_kernels_did_not_run(nat, staged, ri):
    import torch

    row = ROWS[ri]
    N, _, (A, M, d, *_rest) = row
    inp, st, rd, rix, _, _ = staged.get(row)
    nbytes = _ws_bytes(nat, row)
    ws_t, ws = tfd._filled(nbytes, PATTERN)
    off = ws - ws_t.data_ptr()
    ws_t[off:off + 256] = 0                                  # the tickets: zero between launches, whoever owns the rest
    torch.cuda.synchronize()
    got = staged.call(row, PRUNE | LISTS_ONLY, ws_t, ws, nbytes)
    assert np.array_equal(got["idx"], rix) and np.array_equal(got["dist"], rd) and got["tickets_zero"]
    # the digit planes of W: the first field behind the tickets, 3 x Mpad x dpad bytes (whole 512-prototype chunks,
    # whole 64-feature k-tiles, two at least)
    Mpad, dpad = (M + 511) // 512 * 512, max((d + 63) // 64 * 64, 128)
    planes = tfd._bytes_at(ws_t, ws + 256, 3 * Mpad * dpad)
    assert (planes == PATTERN).all(), "slice_w_tiled_kernel ran"
    gaps = np.zeros((M, M), dtype=np.float32)
    nat.call("dbgsom_bmu_filtered_gaps", ws, N, d, M, gaps.ctypes.data, da.stream())
    assert (gaps.view(np.uint8) == PATTERN).all(), "proto_gap_kernel ran"
    assert (got["seed"].view(np.uint8) == PATTERN).all(), "anchor_gather_kernel ran"
    assert an.check_argmin(got["aseed"], inp["anchors"], inp["W"]) == A      # aseed is written
    assert (got["counts"] >= 1).all() and (got["counts"] <= M).all()
    assert (tfd._bytes_at(ws_t, ws + nbytes, 256) == PATTERN).all()          # nothing behind the workspace's end


# ---- 3. the seed kernel at the edges of its split of k -----------------------------------------------------------------
@pytest.mark.parametrize("A", [17, 256])
@pytest.mark.parametrize("M", [20, 130, 1985])
@pytest.mark.parametrize("d", [16, 48, 208])
def test_seed_kernel_at_the_edges_of_the_k_split(nat, o, d, M, A):
    """d / 16 = 1, 3 and 13 k-steps over four wavefronts: 1/0/0/0, 1/1/1/0 and 4/3/3/3"""
    X, W = am.blobs(300, d, M, "ksplit")
    got = tamd.run_case(nat, o, X, W, "f32", A=A)
    assert got["anchors"].shape[0] == A
    assert an.check_argmin(got["aseed"], got["anchors"], got["Wp"]) == A
    tamd.check_bounds(got)
    tamd.check_exact(o, got)
    lean = tamd.run_case(nat, o, X, W, "f32", A=A, flags=PRUNE | LISTS_ONLY)
    assert np.array_equal(lean["aseed"], got["aseed"]) and np.array_equal(lean["low"], got["low"])
    assert np.array_equal(lean["up"], got["up"])
    tamd.check_lists(lean)
    tamd.check_exact(o, lean)
