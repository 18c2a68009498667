"""MI355X: the filtered search at device level (tests/filter_device.py holds the tables and the checks).

1. dbgsom_filter_prepare against the emulation the proof of tests/test_filter_bound.py works on: digit planes and
   scales bit for bit, l1 and the 16-bit residual inside their certified directions.
2. The gap table of the triangle-inequality form (read with dbgsom_bmu_filtered_gaps): a lower bound of every squared
   prototype distance in direct form, symmetric, 0 where nothing is known, and not vacuous where the emulation is clear.
3. dbgsom_bmu_filtered called raw over a pairwise table of shapes, types, strides, flags and seeds, every case in ONE
   workspace zero-filled once (table order, then reversed) and in a fresh one: winners and distances equal
   oracle.som_oracle.bmu_chain bit for bit, the tickets are back at zero after every call."""
import numpy as np
import pytest

from tests import device_abi as da
from tests import filter_device as fd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


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


def _filled(nbytes, byte):
    """-> (tensor, 256-byte aligned pointer) of `nbytes` bytes and 256 more behind them, all `byte`"""
    t = _full((int(nbytes) + 512,), byte, "uint8")
    return t, (t.data_ptr() + 255) // 256 * 256


def _bytes_at(t, ptr, n):
    off = ptr - t.data_ptr()
    return t[off:off + n].cpu().numpy()


# ---- 1. dbgsom_filter_prepare ---------------------------------------------------------------------------------------
def _prepare(nat, A, ld, off, dtype):
    """dbgsom_filter_prepare on the staged rows of A (as stored) -> (planes, scale, l1, res16) on the host; the buffer
    starts as 0x7f bytes, and the bytes behind its end must stay that"""
    rows, d = A.shape
    _keep, ptr = da.stage(A, ld, off, dtype)
    total = nat.load().dbgsom_filter_planes_bytes(rows, d)
    assert total == fd.planes_layout(rows, d)["total"]
    buf, bptr = _filled(total, 0x7f)
    nat.call("dbgsom_filter_prepare", ptr, da.CODE[dtype], rows, d, ld, bptr, total, da.stream())
    _sync()
    host = _bytes_at(buf, bptr, total + 256)
    assert (host[total:] == 0x7f).all()
    return fd.split_planes(host, rows, d)


@pytest.mark.parametrize("d", fd.PREP_D)
@pytest.mark.parametrize("rows", fd.PREP_ROWS)
@pytest.mark.parametrize("dtype", fd.PREP_DTYPES)
def test_filter_prepare_equals_the_emulation(nat, dtype, rows, d):
    A = fd.prepare_rows(rows, d, dtype)
    Aw = np.asarray(da.widen(A), dtype=np.float64)
    first = None
    for pad, off in fd.PREP_LAYOUTS:
        got = _prepare(nat, A, d + pad, off, dtype)
        if first is None:
            first = got
            worst_l1, worst_res = fd.check_prepared(Aw, *got)
            print(f"prepare {dtype} rows={rows} d={d}: l1 error / bound {worst_l1:.3f}, res16 / |a - a16| <= {worst_res:.12f}")
            if rows >= 5:
                fd.check_special_rows(Aw, got[0], got[1], got[2], 0)
            if rows >= 131:
                fd.check_special_rows(Aw, got[0], got[1], got[2], rows - 4)
        else:                                   # the row stride and the base address change no bit
            for a, b in zip(first, got):
                assert np.array_equal(a, b), (pad, off)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("rows,d", [(5, 16), (5, 200), (131, 65), (131, 128)])
@pytest.mark.parametrize("dtype", fd.PREP_DTYPES)
def test_filter_prepare_row_with_a_nan_or_an_infinity(nat, dtype, rows, d, bad):
    A = np.asarray(da.widen(fd.prepare_rows(rows, d, dtype)), dtype=np.float64)
    r = rows // 2
    B, Z = A.copy(), A.copy()
    B[r, d // 3] = bad
    Z[r] = 0.0
    got = _prepare(nat, da.stored(B, dtype), d + 3, 1, dtype)
    ref = _prepare(nat, da.stored(Z, dtype), d + 3, 1, dtype)
    assert np.isnan(got[3][r]), "res16 of a row with a NaN or an infinity must be NaN (no bound)"
    others = np.arange(rows) != r
    assert np.array_equal(got[0][:, others], ref[0][:, others])
    for a, b in zip(got[1:], ref[1:]):
        assert np.array_equal(a[others], b[others])
    fd.check_prepared(Z, *ref, rows_to_check=np.flatnonzero(others))


# ---- the raw filtered call ------------------------------------------------------------------------------------------
def _norms(nat, ptr, code, rows, d, ld):
    out = _full((rows,), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, code, rows, d, ld, out.data_ptr(), da.stream())
    return out


def _stage_search(nat, X, W, ldx, dtype):
    """everything a raw dbgsom_bmu_filtered call reads: the staged rows (NaN in the columns d .. ldx), xx and ww from
    dbgsom_row_sqnorms, the planes from dbgsom_filter_prepare on the same staged rows"""
    N, d = X.shape
    M = W.shape[0]
    xt, xptr = da.stage(X, ldx, 0, dtype)
    wt = da.dev(W)
    xx = _norms(nat, xptr, da.CODE[dtype], N, d, ldx)
    ww = _norms(nat, wt.data_ptr(), da.F64, M, d, d)
    pbytes = nat.load().dbgsom_filter_planes_bytes(N, d)
    pt, pptr = _filled(pbytes, 0x7f)
    nat.call("dbgsom_filter_prepare", xptr, da.CODE[dtype], N, d, ldx, pptr, pbytes, da.stream())
    _sync()
    return {"keep": (xt, wt, xx, ww, pt), "x": xptr, "code": da.CODE[dtype], "N": N, "d": d, "ldx": ldx, "xx": xx.data_ptr(),
            "planes": pptr, "W": wt.data_ptr(), "M": M, "ww": ww.data_ptr()}


def _workspace_bytes(nat, N, d, M):
    n = nat.load().dbgsom_bmu_filtered_workspace_bytes(N, d, M)
    assert n > 256
    return n


def _search(nat, st, flag_arg, planes, round_f32, prev, order, ws_t, ws, ws_bytes):
    """one dbgsom_bmu_filtered call -> dict: idx, dist, whether the tickets are zero behind it, the list lengths of
    the workgroups, the refinement's counters (DBGSOM_REFINE calls)"""
    N, d, M = st["N"], st["d"], st["M"]
    idx, dist = _full((N,), -7, "int64"), _full((N,), float("nan"), "float64")
    prev_t = da.dev(prev) if prev is not None else None
    order_t = da.dev(order) if order is not None else None
    nat.call("dbgsom_bmu_filtered", st["x"], st["code"], N, d, st["ldx"], st["xx"], st["planes"], st["W"], M, st["ww"],
             prev_t.data_ptr() if prev is not None else None, order_t.data_ptr() if order is not None else None,
             flag_arg, planes, round_f32, idx.data_ptr(), dist.data_ptr(), ws, ws_bytes, da.stream())
    _sync()
    out = {"idx": idx.cpu().numpy(), "dist": dist.cpu().numpy(), "tickets_zero": not _bytes_at(ws_t, ws, 256).any()}
    nb = (N + 127) // 128
    counts = np.full(nb, 0xffffffff, dtype=np.uint32)
    nat.call("dbgsom_bmu_filtered_counts", ws, N, d, M, counts.ctypes.data, nb, da.stream())
    out["counts"] = counts.astype(np.int64)
    if flag_arg & fd.REFINE:
        out4 = np.zeros(4, dtype=np.uint64)
        nat.call("dbgsom_bmu_filtered_refine_counts", ws, N, d, M, out4.ctypes.data, da.stream())
        out["refine"] = out4
    return out


# ---- 2. the gap table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bad", fd.GAP_INPUTS)
@pytest.mark.parametrize("M,d", fd.GAP_SHAPES)
def test_gap_table_is_a_lower_bound_and_not_an_empty_one(nat, o, M, d, name, bad):
    X, W = fd.gap_inputs(name, M, d, bad)
    ref = fd.gap_reference(W)
    rd, ri = o.bmu_chain(X, W, 1)
    st = _stage_search(nat, X, W, d, "f32")
    nbytes = _workspace_bytes(nat, fd.GAP_N, d, M)
    tables = []
    for mode, flag in (("prune", fd.PRUNE), ("probe", fd.PRUNE_PROBE)):
        ws_t, ws = da.workspace(nbytes)
        got = _search(nat, st, flag, 0, 0, None, None, ws_t, ws, nbytes)
        gap = np.full((M, M), np.nan, dtype=np.float32)
        nat.call("dbgsom_bmu_filtered_gaps", ws, fd.GAP_N, d, M, gap.ctypes.data, da.stream())
        worst, clear = fd.check_gap_table(gap, W, ref)
        print(f"gap table M={M} d={d} {name}{' +nan/inf rows' if bad else ''} {mode}: worst gap / exact {worst:.4f}, "
              f"clear pairs {clear:.5f}")
        assert worst <= 1.0
        assert np.array_equal(got["idx"], ri) and np.array_equal(got["dist"], rd), mode
        assert got["tickets_zero"]
        fd.check_counts(got["counts"], fd.GAP_N, M, None, ri)
        tables.append(gap)
    assert np.array_equal(tables[0], tables[1])          # the same kernel on the same planes, whichever form asked for it


# ---- 3. dbgsom_bmu_filtered over the pairwise table -------------------------------------------------------------------
class _RawCases:
    """staged inputs per (shape, type, row stride), references and seeds per case: built once, on first use"""

    def __init__(self, nat, o):
        self.nat, self.o = nat, o
        self.data, self.staged, self.refs = {}, {}, {}

    def inputs(self, si, dtype):
        if (si, dtype) not in self.data:
            X, W = fd.raw_data(si, dtype)
            rd, ri = self.o.bmu_chain(X, W.astype(np.float32) if dtype == "f32r" else W, 1)
            self.data[(si, dtype)] = (X, W, rd, ri)
        return self.data[(si, dtype)]

    def stage(self, si, dtype, pad):
        key = (si, dtype, pad)
        if key not in self.staged:
            X, W, _, _ = self.inputs(si, dtype)
            self.staged[key] = _stage_search(self.nat, X, W, X.shape[1] + pad, "f64" if dtype == "f64" else "f32")
        return self.staged[key]

    def run(self, ci, ws_t, ws, ws_bytes):
        case = fd.RAW_CASES[ci]
        si, dtype, pad, planes, stride, flags, seeds = case
        N, d, M, _, ldx, flag_arg, planes, round_f32, hinted = fd.raw_call_args(case)
        X, W, rd, ri = self.inputs(si, dtype)
        prev, order = fd.raw_seeds(seeds, X, W, ri, ci)
        st = self.stage(si, dtype, pad)
        assert (st["N"], st["d"], st["M"], st["ldx"]) == (N, d, M, ldx)
        out = _search(self.nat, st, flag_arg, planes, round_f32, prev, order, ws_t, ws, ws_bytes)
        out["order"] = order
        return out


@pytest.fixture(scope="module")
def raw(nat, o):
    return _RawCases(nat, o)


@pytest.fixture(scope="module")
def shared_runs(nat, raw):
    """every case in ONE workspace, sized for the largest and zero-filled once: table order, then reversed"""
    sizes = [_workspace_bytes(nat, *fd.RAW_SHAPES[c[0]]) for c in fd.RAW_CASES]
    ws_t, ws = da.workspace(max(sizes))
    runs = {}
    n = len(fd.RAW_CASES)
    for tag, seq in (("forward", range(n)), ("reverse", range(n - 1, -1, -1))):
        for ci in seq:
            runs[(tag, ci)] = raw.run(ci, ws_t, ws, sizes[ci])
    return runs


@pytest.mark.parametrize("ci", range(len(fd.RAW_CASES)), ids=["-".join(map(str, c)) for c in fd.RAW_CASES])
def test_bmu_filtered_raw(nat, raw, shared_runs, ci):
    case = fd.RAW_CASES[ci]
    N, d, M = fd.RAW_SHAPES[case[0]]
    _, _, rd, ri = raw.inputs(case[0], case[1])
    nbytes = _workspace_bytes(nat, N, d, M)
    ws_t, ws = da.workspace(nbytes)
    fresh = raw.run(ci, ws_t, ws, nbytes)
    for tag, got in (("fresh", fresh), ("forward", shared_runs[("forward", ci)]), ("reverse", shared_runs[("reverse", ci)])):
        assert np.array_equal(got["idx"], ri), (tag, int((got["idx"] != ri).sum()))
        assert np.array_equal(got["dist"], rd), (tag, int((got["dist"] != rd).sum()))
        assert got["tickets_zero"], tag
        fd.check_counts(got["counts"], N, M, got["order"], ri)
        if "refine" in got:
            fd.check_refine_counts(got["refine"], N, M)
    if case[1] == "f32r":
        assert np.array_equal(rd, rd.astype(np.float32).astype(np.float64))
    if case[6] == "dup_hi" and M >= 8:
        prev, _ = fd.raw_seeds("dup_hi", *raw.inputs(case[0], case[1])[:2], ri, ci)
        assert (prev > ri).any()                  # some seeds ARE higher-indexed copies: the tie still went to the lowest
