"""MI355X: addresses more than 2^32 bytes from the pointer a call is given.

Part A: the raw entry points of include/dbgsom_hip.h on 35 rows placed 2^28 bytes apart in one 9 GiB allocation
(tests/large_offsets.py): rows 8+ past byte 2^31, 16+ past 2^32, 32+ past 2^33 and, for the narrow types, past
element 2^31 / 2^32.  The allocation holds 0xff bytes (NaN / -1) around the rows: a read of anything but a row's d
values poisons the result.  Results that take a leading dimension land in the same allocation, 2^20 bytes behind
each row.  Every result is compared with the CPU reference the project already has for that call, and -- where the
kernel chosen does not depend on the stride -- bit for bit with the same call on the same rows stored compactly.

Part B: tall compact matrices (more than 2^31 float32 and more than 2^32 bfloat16 elements) through the context
and the raw sums.

No test asserts on a clock."""
import time
from math import fsum as math_fsum

import numpy as np
import pytest

from tests import cosine as cs
from tests import device_abi as da
from tests import kneighbors as kn
from tests import large_offsets as lo
from tests import manhattan as mh
from tests import masked_fit as mf
from tests import prototype_distances as pd
from tests.test_missing_cpu import RTOL, fill_numpy, masked_distances, winners_of

pytestmark = pytest.mark.gpu

T0 = time.monotonic()


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


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a fault of the device is sticky: nothing more of this module is started on it"""
    import torch

    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an earlier fault, the module ends here: {e}", returncode=3)
    yield


def _full(shape, value, dtype):
    import torch

    return torch.full(shape, value, dtype=getattr(torch, dtype), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _need(nbytes):
    """skip (with the two numbers) when the card cannot give `nbytes` more"""
    import torch

    free, _total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{nbytes} bytes of device memory needed, {free} free")


# ---- the far allocation ------------------------------------------------------------------------------------------------
class Far:
    """the 9 GiB allocation of part A"""
    TORCH = {"f32": "float32", "f64": "float64", "bf16": "int16"}

    def __init__(self):
        import torch

        _need(lo.TOTAL + 2 ** 30)
        self.buf = torch.empty(lo.TOTAL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.base = self.buf.data_ptr()
        self.words = self.buf.view(torch.int64)

    def fill(self):
        self.words.fill_(-1)            # 0xff bytes: NaN for every float type, -1 for every integer

    def _strided(self, tdtype, item, ld, cols, byte0, rows):
        import torch

        v = self.buf.view(getattr(torch, tdtype))
        assert byte0 % item == 0
        return torch.as_strided(v, (rows, cols), (ld, 1), byte0 // item)

    def rows(self, geom, d, rows=lo.ROWS):
        """the strided view of the input rows' d values"""
        dtype = lo.dtype_of(geom)
        return self._strided(self.TORCH[dtype], da.ITEM[dtype], lo.ld_of(geom), d, 0, rows)

    def put(self, geom, A):
        """fill with 0xff, write the rows of A (as da.stored returns them) -> the pointer of row 0"""
        import torch

        self.fill()
        src = torch.from_numpy(A.view(np.int16) if A.dtype == np.uint16 else A).cuda()
        self.rows(geom, A.shape[1], A.shape[0]).copy_(src)
        return self.base

    def window(self, geom, cols, tdtype="float64", item=8, rows=lo.ROWS):
        """the strided view of the output windows (`cols` elements of `item` bytes behind every row)"""
        assert cols * item <= lo.WINDOW
        return self._strided(tdtype, item, lo.out_ld(geom, item), cols, lo.WINDOW, rows)

    def window_ptr(self):
        return self.base + lo.WINDOW

    def untouched_outside(self, views):
        """every byte outside `views` still holds 0xff (the views are overwritten with 0xff on the way)"""
        import torch

        for v in views:
            if v.dtype.is_floating_point:       # (a NaN of all-one bits; a copy within one dtype moves the bits as they are)
                ones = torch.full((1,), -1, dtype=torch.int64 if v.element_size() == 8 else torch.int32, device="cuda")
                v.copy_(ones.view(v.dtype).expand_as(v))
            else:
                v.fill_(-1)
        step = 2 ** 27
        for a in range(0, self.words.numel(), step):
            if bool((self.words[a:a + step] != -1).any()):
                return False
        return True


@pytest.fixture(scope="module")
def far():
    import torch

    f = Far()
    yield f
    del f.words, f.buf
    torch.cuda.empty_cache()


def _compact_ld(geom, d, same_class):
    """a small stride whose rows fall into the same kernel class as the far ones (same_class(ld) -> bool)"""
    for ld in (d, d + 1, d + 2, d + 4, d + 8):
        if same_class(ld):
            return ld
    raise AssertionError(f"{geom}: no compact stride of the same class")


def _norms_at(nat, ptr, dtype, rows, d, ld):
    out = _full((rows,), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], rows, d, ld, out.data_ptr(), da.stream())
    return out


def _w_dev(nat, W):
    """contiguous float64 prototypes and their norms on the device -> (tensor, norms tensor)"""
    wt = da.dev(np.ascontiguousarray(W, dtype=np.float64))
    ww = _norms_at(nat, wt.data_ptr(), "f64", W.shape[0], W.shape[1], W.shape[1])
    return wt, ww


def _protos(M, d, seed, f32=False):
    W = np.random.default_rng(seed).normal(size=(M, d)) * 1.5
    return W.astype(np.float32).astype(np.float64) if f32 else W


# ---- A1. dbgsom_row_sqnorms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,d", lo.NORM_CASES, ids=["%s-d%d" % c for c in lo.NORM_CASES])
def test_row_sqnorms_far_rows(nat, o, far, geom, d):
    dtype, ld = lo.GEOM[geom]
    A = lo.random_rows(geom, d, 11 + d)
    out = _norms_at(nat, far.put(geom, A), dtype, lo.ROWS, d, ld)
    _sync()
    assert np.array_equal(out.cpu().numpy(), o.row_sqnorms_chain(da.widen(A)))


# ---- A2. dbgsom_bmu -----------------------------------------------------------------------------------------------------
def _bmu_at(nat, xptr, dtype, N, d, ldx, W, k):
    wt, ww = _w_dev(nat, W)
    xx = _norms_at(nat, xptr, dtype, N, d, ldx)
    idx, dist = _full((N, k), -7, "int64"), _full((N, k), float("nan"), "float64")
    nat.call("dbgsom_bmu", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wt.data_ptr(), W.shape[0], ww.data_ptr(), k, 0,
             idx.data_ptr(), dist.data_ptr(), da.stream())
    _sync()
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    return (dist.reshape(-1), idx.reshape(-1)) if k == 1 else (dist, idx)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("geom,d,M,cls", lo.BMU_CASES, ids=lo.BMU_IDS)
def test_bmu_far_rows(nat, o, far, geom, d, M, cls, k):
    dtype, ld = lo.GEOM[geom]
    assert da.bmu_class(dtype, d, ld, 0, 0, M)[0] == cls
    X, W = lo.random_rows(geom, d, 100 + d + M, 2.0), _protos(M, d, M + d)
    dist, idx = _bmu_at(nat, far.put(geom, X), dtype, lo.ROWS, d, ld, W, k)
    rd, ri = o.bmu_chain(da.widen(X), W, k)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    ldc = _compact_ld(geom, d, lambda c: da.bmu_class(dtype, d, c, 0, 0, M) == da.bmu_class(dtype, d, ld, 0, 0, M))
    _xt, xptr = da.stage(X, ldc, 0, dtype)
    cd, ci = _bmu_at(nat, xptr, dtype, lo.ROWS, d, ldc, W, k)
    assert np.array_equal(ci, idx) and np.array_equal(_bits(cd), _bits(dist))


# ---- A3. column sums ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,d", lo.COLSUM_CASES, ids=["%s-d%d" % c for c in lo.COLSUM_CASES])
def test_column_sums_far_rows(nat, far, geom, d):
    dtype, ld = lo.GEOM[geom]
    X = lo.random_rows(geom, d, 7 + d, 2.0)
    xptr = far.put(geom, X)
    mean = (da.column_sums_loop(X) / X.dtype.type(lo.ROWS)).astype(X.dtype)
    mean_t = da.dev(mean)
    for m_ptr, m in ((None, None), (mean_t.data_ptr(), mean)):
        out = da.dev(np.full(d, np.nan, dtype=X.dtype))
        nat.call("dbgsom_column_sums", xptr, da.CODE[dtype], lo.ROWS, d, ld, m_ptr, out.data_ptr(), da.stream())
        _sync()
        assert np.array_equal(out.cpu().numpy(), da.column_sums_loop(X, m))


@pytest.mark.parametrize("geom,d", lo.WCOLSUM_CASES, ids=["%s-d%d" % c for c in lo.WCOLSUM_CASES])
def test_weighted_column_sums_far_rows(nat, far, geom, d):
    """within (N + 2) u sum |terms| of the longdouble sums, as tests/test_gpu_device_abi.py derives it, and the bits of
    the same call on compact rows (the kernel has one form)"""
    dtype, ld = lo.GEOM[geom]
    N = lo.ROWS
    X = da.stored(np.asarray(da.widen(lo.random_rows(geom, d, 9 + d, 2.0)), dtype=np.float32), dtype)
    Xw = np.asarray(da.widen(X), dtype=np.float64)
    rng = np.random.default_rng(d)
    w = rng.integers(0, 4, N).astype(np.float64) * rng.uniform(0.1, 2.5, N)
    w[-1] = 1.75                                                    # the last row counts
    mean = Xw.mean(axis=0).astype(np.float32).astype(np.float64)
    w_t, mean_t = da.dev(w), da.dev(mean)
    nbytes = nat.load().dbgsom_weighted_column_sums_workspace_bytes(d)
    _ws, ws = da.workspace(nbytes)
    xptr = far.put(geom, X)
    _ct, cptr = da.stage(X, d + 3, 0, dtype)
    L = np.longdouble
    for m_ptr, m in ((None, None), (mean_t.data_ptr(), mean)):
        got = []
        for ptr, ldx in ((xptr, ld), (cptr, d + 3)):
            out = _full((d,), float("nan"), "float64")
            nat.call("dbgsom_weighted_column_sums", ptr, da.CODE[dtype], N, d, ldx, w_t.data_ptr(), m_ptr, out.data_ptr(),
                     ws, nbytes, da.stream())
            _sync()
            got.append(out.cpu().numpy())
        base = Xw.astype(L) if m is None else (Xw.astype(L) - m.astype(L)) ** 2
        terms = w.astype(L)[:, None] * base
        ref, T = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        err = np.abs(got[0].astype(L) - ref)
        bound = (N + 2) * da.U * T + 2 * N * da.UL * T
        print(f"largest error / bound {float(np.max(err / np.where(bound > 0, bound, 1))):.3f}")
        assert np.all(err <= bound)
        assert np.array_equal(_bits(got[0]), _bits(got[1]))


# ---- A4. dbgsom_accumulate / _weighted / _masked --------------------------------------------------------------------------
def _accumulate_at(nat, xptr, dtype, N, d, ldx, winners, kw, dist, M, sw=None):
    """-> ((S, K, a, E), status, order)"""
    lib = nat.load()
    win_t, kw_t, dist_t = da.dev(winners), da.dev(kw), da.dev(dist)
    sw_t = da.dev(sw) if sw is not None else None
    name = "dbgsom_accumulate_weighted" if sw is not None else "dbgsom_accumulate"
    nbytes = getattr(lib, name + "_workspace_bytes")(N, d, M)
    assert nbytes > 0
    ws_t, ws = da.workspace(nbytes)
    sums = _full((M * (d + 3),), float("nan"), "float64")
    st = _full((1,), 77, "int32")
    args = [xptr, da.CODE[dtype], N, d, ldx, win_t.data_ptr(), kw_t.data_ptr()]
    if sw is not None:
        args.append(sw_t.data_ptr())
    args += [dist_t.data_ptr(), M, sums.data_ptr(), st.data_ptr(), ws, nbytes, da.stream()]
    nat.call(name, *args)
    _sync()
    v = sums.cpu().numpy()
    skip = ws - ws_t.data_ptr()
    order = ws_t[skip:skip + 4 * N].cpu().numpy().view(np.int32)
    return (v[:M * d].reshape(M, d), v[M * d:M * d + M], v[M * d + M:M * d + 2 * M], v[M * d + 2 * M:]), int(st.cpu()[0]), order


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("geom,d,cls", lo.SEGSUM_CASES, ids=lo.SEGSUM_IDS)
def test_accumulate_far_rows(nat, far, geom, d, cls, weighted):
    dtype, ld = lo.GEOM[geom]
    N, M = lo.ROWS, lo.ACC_M
    assert da.segsum_class(dtype, d, ld, 0) == cls
    rng = np.random.default_rng(d + len(geom))
    winners = lo.acc_winners(rng)
    winners[-1] = 3                                             # (the far end belongs to a neuron with other rows)
    counts = np.bincount(winners, minlength=M)
    assert counts[1] == 0
    X = lo.random_rows(geom, d, 300 + d)
    kw, dist = 1.0 - rng.random(N), 3.0 * rng.random(N)
    sw = None
    if weighted:
        sw = rng.integers(0, 4, N).astype(np.float64)
        sw[-1] = 2.0
    (S, K, a, E), st, order = _accumulate_at(nat, far.put(geom, X), dtype, N, d, ld, winners, kw, dist, M, sw)
    (Sr, Kr, ar, Er), (TS, TK, TE) = da.accumulate_reference(da.widen(X), winners, kw, dist, M, sw)
    assert st == 0 and not any(np.isnan(p).any() for p in (S, K, a, E))
    if sw is None:
        assert np.array_equal(a, counts)
    else:
        assert np.array_equal(a, np.bincount(winners, weights=sw, minlength=M))
    for name, got, ref, T in (("S", S, Sr, TS), ("K", K, Kr, TK), ("E", E, Er, TE)):
        ok, r = da.sums_within_bound(got, ref, T, counts, sw is not None)
        print(f"{name}: largest error / bound {r:.3f}")
        assert ok, name
    assert (S[1] == 0).all() and K[1] == 0 and E[1] == 0 and a[1] == 0
    assert np.array_equal(order, np.argsort(winners, kind="stable"))
    ldc = _compact_ld(geom, d, lambda c: da.segsum_class(dtype, d, c, 0) == cls)
    _xt, cptr = da.stage(X, ldc, 0, dtype)
    (Sc, Kc, ac, Ec), stc, _ = _accumulate_at(nat, cptr, dtype, N, d, ldc, winners, kw, dist, M, sw)
    assert all(np.array_equal(_bits(g), _bits(c)) for g, c in ((S, Sc), (K, Kc), (a, ac), (E, Ec)))


def _punched(geom, d, seed, frac=0.3):
    """random float32 / float64 rows with holes (NaN), one observed cell per row at least"""
    rng = np.random.default_rng(seed)
    X = np.array(lo.random_rows(geom, d, seed, 2.0))
    holes = rng.random(X.shape) < frac
    holes[np.arange(len(X)), rng.integers(0, d, len(X))] = False
    X[holes] = np.nan
    return X


@pytest.mark.parametrize("geom", lo.MASKED_GEOMS)
def test_accumulate_masked_far_rows(nat, far, geom):
    dtype, ld = lo.GEOM[geom]
    assert ld <= lo.MASKED_LD_CAP
    N, M, d = lo.ROWS, lo.ACC_M, 37
    rng = np.random.default_rng(len(geom))
    winners = lo.acc_winners(rng)
    X = _punched(geom, d, 41)
    kw, dist = 1.0 - rng.random(N), 3.0 * rng.random(N)
    win_t, kw_t, dist_t = da.dev(winners), da.dev(kw), da.dev(dist)
    nbytes = nat.load().dbgsom_accumulate_masked_workspace_bytes(N, d, M)
    _ws, ws = da.workspace(nbytes)
    got = []
    ldc = lo.same_alignment_ld(geom, d)
    assert da.aligned16(ldc, 0, dtype) == lo.aligned16(geom)
    _ct, cptr = da.stage(X, ldc, 0, dtype)
    for ptr, ldx in ((far.put(geom, X), ld), (cptr, ldc)):
        sums = _full((M * (3 * d + 2),), float("nan"), "float64")
        st = _full((1,), 77, "int32")
        nat.call("dbgsom_accumulate_masked", ptr, da.CODE[dtype], N, d, ldx, win_t.data_ptr(), kw_t.data_ptr(),
                 dist_t.data_ptr(), M, sums.data_ptr(), st.data_ptr(), ws, nbytes, da.stream())
        _sync()
        assert int(st.cpu()[0]) == 0
        got.append(sums.cpu().numpy())
    Md = M * d
    v = got[0]
    S, K, A, a, E = v[:Md].reshape(M, d), v[Md:2 * Md].reshape(M, d), v[2 * Md:3 * Md].reshape(M, d), v[3 * Md:3 * Md + M], v[3 * Md + M:]
    (Sr, Kr, Ar, ar, Er), (TS, TK, TE) = mf.masked_sums_longdouble(X, winners, kw, dist, M)
    assert np.array_equal(A, Ar) and np.array_equal(a, ar) and a.sum() == N
    for label, g, ref, T, n in (("S", S, Sr, TS, A), ("K", K, Kr, TK, A), ("E", E, Er, TE, a)):
        n_ = np.asarray(n, dtype=np.longdouble)
        bound = (n_ + 2) * da.U * T + n_ * da.UL * T
        assert np.all(np.abs(np.asarray(g, dtype=np.longdouble) - ref) <= bound), label
    assert np.array_equal(_bits(got[0]), _bits(got[1]))


# ---- A5. rows with missing entries: dbgsom_bmu_masked, dbgsom_fill_missing ------------------------------------------------
def _bmu_masked_at(nat, xptr, dtype, N, d, ldx, wt, M, k):
    nbytes = nat.load().dbgsom_bmu_masked_workspace_bytes(da.CODE[dtype], N, d, M)
    _ws, ws = da.workspace(nbytes)
    idx, dist = _full((N, k), -7, "int64"), _full((N, k), float("nan"), "float64")
    nat.call("dbgsom_bmu_masked", xptr, da.CODE[dtype], N, d, ldx, wt.data_ptr(), M, d, k, idx.data_ptr(), dist.data_ptr(),
             ws, nbytes, da.stream())
    _sync()
    return dist.cpu().numpy(), idx.cpu().numpy(), idx


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("geom", lo.MASKED_GEOMS)
def test_bmu_masked_and_fill_missing_far_rows(nat, far, geom, k):
    dtype, ld = lo.GEOM[geom]
    N, d, M = lo.ROWS, 37, 9
    X, W = _punched(geom, d, 51), _protos(M, d, 5)
    wt = da.dev(W)
    xptr = far.put(geom, X)
    dist, idx, idx_t = _bmu_masked_at(nat, xptr, dtype, N, d, ld, wt, M, k)
    D = masked_distances(X, W)
    wd, wi = winners_of(D, k)
    assert np.array_equal(idx.reshape(wi.shape), wi)
    np.testing.assert_allclose(dist.reshape(wd.shape), wd, rtol=RTOL, atol=0.0)
    _ct, cptr = da.stage(X, d, 0, dtype)
    cd, ci, _ = _bmu_masked_at(nat, cptr, dtype, N, d, d, wt, M, k)
    assert np.array_equal(ci, idx) and np.array_equal(_bits(cd), _bits(dist))
    # the fill writes into the far rows: the holes get the winner's entries, nothing else changes
    nat.call("dbgsom_fill_missing", xptr, da.CODE[dtype], N, d, ld, wt.data_ptr(), M, d, idx_t.data_ptr(), k, da.stream())
    _sync()
    rows = far.rows(geom, d)
    filled = rows.cpu().numpy()
    assert np.array_equal(filled, fill_numpy(X, W, idx[:, 0]))
    assert far.untouched_outside([rows])


# ---- A6. the distance matrices: far ldx and far ldo ------------------------------------------------------------------------
def _dist_window(far, geom, M):
    out = far.window(geom, M)
    return out, far.window_ptr(), lo.out_ld(geom)


@pytest.mark.parametrize("geom,d,M", lo.DIST_CASES, ids=lo.DIST_IDS)
def test_distances_far_rows_and_far_result(nat, far, geom, d, M):
    dtype, ld = lo.GEOM[geom]
    N = lo.ROWS
    X, W = lo.random_rows(geom, d, 600 + d, 2.0), _protos(M, d, 60 + M)
    xptr = far.put(geom, X)
    wt, ww = _w_dev(nat, W)
    xx = _norms_at(nat, xptr, dtype, N, d, ld)
    out, optr, ldo = _dist_window(far, geom, M)
    nat.call("dbgsom_distances", xptr, da.CODE[dtype], N, d, ld, xx.data_ptr(), wt.data_ptr(), M, ww.data_ptr(), optr, ldo,
             da.stream())
    _sync()
    D = out.cpu().numpy()
    assert np.array_equal(D, pd.pair_distances(X, W))
    assert far.untouched_outside([out, far.rows(geom, d)])


@pytest.mark.parametrize("form", ["masked", "manhattan"])
@pytest.mark.parametrize("M", [3, 513])
@pytest.mark.parametrize("geom", [g for g in lo.MASKED_GEOMS if g in lo.OUT_GEOMS])
def test_direct_form_distances_far_rows_and_far_result(nat, far, geom, M, form):
    dtype, ld = lo.GEOM[geom]
    assert ld <= lo.MASKED_LD_CAP
    N, d = lo.ROWS, 37
    W = _protos(M, d, 70 + M)
    X = _punched(geom, d, 71) if form == "masked" else np.array(lo.random_rows(geom, d, 72, 2.0))
    wt = da.dev(W)
    xptr = far.put(geom, X)
    out, optr, ldo = _dist_window(far, geom, M)
    size = getattr(nat.load(), "dbgsom_bmu_%s_workspace_bytes" % form)(da.CODE[dtype], N, d, M)
    _ws, ws = da.workspace(size)
    nat.call("dbgsom_distances_" + form, xptr, da.CODE[dtype], N, d, ld, wt.data_ptr(), M, d, optr, ldo, ws, size, da.stream())
    _sync()
    D = out.cpu().numpy()
    if form == "masked":
        np.testing.assert_allclose(D, masked_distances(X, W), rtol=RTOL, atol=0.0)
    else:
        assert np.array_equal(D, mh.l1_distances(X, W))
    assert far.untouched_outside([out, far.rows(geom, d)])


def _cosine_parts(nat, xptr, dtype, N, d, ld, W):
    """u, v of the cosine calls: inverse norms of the rows at xptr and of W"""
    wt, ww = _w_dev(nat, W)
    xx = _norms_at(nat, xptr, dtype, N, d, ld)
    u, v = _full((N,), float("nan"), "float64"), _full((W.shape[0],), float("nan"), "float64")
    nat.call("dbgsom_inv_norms", xx.data_ptr(), N, u.data_ptr(), da.stream())
    nat.call("dbgsom_inv_norms", ww.data_ptr(), W.shape[0], v.data_ptr(), da.stream())
    return wt, u, v


def _cosine_rows(geom, d, seed):
    """float32-representable rows (the plain multiply-add of tests/cosine.py is then the fma)"""
    A = np.asarray(lo.random_rows(geom, d, seed, 2.0), dtype=np.float32)
    return A.astype(lo.NP_DTYPE[lo.dtype_of(geom)])


@pytest.mark.parametrize("M", [3, 513])
@pytest.mark.parametrize("geom", [g for g in lo.OUT_GEOMS if lo.dtype_of(g) != "bf16"])
def test_cosine_distances_and_search_far_rows(nat, far, geom, M):
    dtype, ld = lo.GEOM[geom]
    N, d = lo.ROWS, 48 if lo.aligned16(geom) else 33
    X, W = _cosine_rows(geom, d, 81), _protos(M, d, 80 + M, f32=True)
    xptr = far.put(geom, X)
    wt, u, v = _cosine_parts(nat, xptr, dtype, N, d, ld, W)
    out, optr, ldo = _dist_window(far, geom, M)
    nat.call("dbgsom_distances_cosine", xptr, da.CODE[dtype], N, d, ld, u.data_ptr(), wt.data_ptr(), M, v.data_ptr(), optr,
             ldo, da.stream())
    found = {}
    for k in (1, 2):
        idx, dist = _full((N, k), -7, "int64"), _full((N, k), float("nan"), "float64")
        nat.call("dbgsom_bmu_cosine", xptr, da.CODE[dtype], N, d, ld, u.data_ptr(), wt.data_ptr(), M, v.data_ptr(), k,
                 idx.data_ptr(), dist.data_ptr(), da.stream())
        found[k] = (dist, idx)
    _sync()
    C = cs.cosine_distances(X, W)
    assert np.array_equal(out.cpu().numpy(), C)
    for k, (dist, idx) in found.items():
        want_dist, want_idx = cs.select(C, k)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(dist.cpu().numpy(), want_dist)
    assert far.untouched_outside([out, far.rows(geom, d)])


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("geom", lo.MASKED_GEOMS)
def test_bmu_manhattan_far_rows(nat, far, geom, k):
    dtype, ld = lo.GEOM[geom]
    N, d, M = lo.ROWS, 37, 300
    X, W = np.array(lo.random_rows(geom, d, 91, 2.0)), _protos(M, d, 90)
    wt = da.dev(W)
    size = nat.load().dbgsom_bmu_manhattan_workspace_bytes(da.CODE[dtype], N, d, M)
    _ws, ws = da.workspace(size)
    _ct, cptr = da.stage(X, d, 0, dtype)
    got = []
    for ptr, ldx in ((far.put(geom, X), ld), (cptr, d)):
        idx, dist = _full((N, k), -7, "int64"), _full((N, k), float("nan"), "float64")
        nat.call("dbgsom_bmu_manhattan", ptr, da.CODE[dtype], N, d, ldx, wt.data_ptr(), M, d, k, idx.data_ptr(),
                 dist.data_ptr(), ws, size, da.stream())
        _sync()
        got.append((dist.cpu().numpy(), idx.cpu().numpy()))
    want_dist, want_idx = mh.l1_select(mh.l1_distances(X, W), k)
    assert np.array_equal(got[0][1], want_idx) and np.array_equal(got[0][0], want_dist)
    assert np.array_equal(got[1][1], got[0][1]) and np.array_equal(_bits(got[1][0]), _bits(got[0][0]))


# ---- A7. the k nearest prototypes: three slabs of the far rows -----------------------------------------------------------
def _kn_results(k):
    return _full((lo.ROWS, k), kn.IDX_SENTINEL, "int64"), _full((lo.ROWS, k), pd.SENTINEL, "float64")


@pytest.mark.parametrize("geom", list(lo.GEOM))
def test_kneighbors_far_rows(nat, far, geom):
    dtype, ld = lo.GEOM[geom]
    N, d, M = lo.ROWS, 48 if lo.aligned16(geom) else 33, lo.KN_M
    X, W = lo.random_rows(geom, d, 700 + d, 2.0), _protos(M, d, 77)
    xptr = far.put(geom, X)
    wt, ww = _w_dev(nat, W)
    xx = _norms_at(nat, xptr, dtype, N, d, ld)
    size = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, lo.KN_SLAB_ROWS)
    _ws, ws = da.workspace(size)
    D = pd.pair_distances(X, W)
    for k in (1, 2, lo.KN_K):
        idx, dist = _kn_results(k)
        nat.call("dbgsom_kneighbors", xptr, da.CODE[dtype], N, d, ld, xx.data_ptr(), wt.data_ptr(), M, ww.data_ptr(), k,
                 lo.KN_SLAB_ROWS, idx.data_ptr(), dist.data_ptr(), ws, size, da.stream())
        _sync()
        want = kn.topk_oracle(X, W, k, D)
        assert np.array_equal(idx.cpu().numpy(), want)
        assert np.array_equal(_bits(dist.cpu().numpy()), _bits(np.take_along_axis(D, want, axis=1)))


@pytest.mark.parametrize("form", ["masked", "manhattan", "cosine"])
@pytest.mark.parametrize("geom", lo.MASKED_GEOMS)
def test_kneighbors_other_metrics_far_rows(nat, far, geom, form):
    dtype, ld = lo.GEOM[geom]
    N, d, M = lo.ROWS, 37, lo.KN_M
    lib = nat.load()
    W = _protos(M, d, 78, f32=True)
    X = {"masked": lambda: _punched(geom, d, 79), "manhattan": lambda: np.array(lo.random_rows(geom, d, 79, 2.0)),
         "cosine": lambda: _cosine_rows(geom, d, 79)}[form]()
    xptr = far.put(geom, X)
    wt = da.dev(W)
    for k in (1, 2, lo.KN_K):
        idx, dist = _kn_results(k)
        if form == "cosine":
            _wt, u, v = _cosine_parts(nat, xptr, dtype, N, d, ld, W)
            size = lib.dbgsom_kneighbors_cosine_workspace_bytes(N, M, lo.KN_SLAB_ROWS)
            _ws, ws = da.workspace(size)
            nat.call("dbgsom_kneighbors_cosine", xptr, da.CODE[dtype], N, d, ld, u.data_ptr(), wt.data_ptr(), M, v.data_ptr(),
                     k, lo.KN_SLAB_ROWS, idx.data_ptr(), dist.data_ptr(), ws, size, da.stream())
        else:
            size = getattr(lib, "dbgsom_kneighbors_%s_workspace_bytes" % form)(da.CODE[dtype], N, d, M, lo.KN_SLAB_ROWS)
            _ws, ws = da.workspace(size)
            nat.call("dbgsom_kneighbors_" + form, xptr, da.CODE[dtype], N, d, ld, wt.data_ptr(), M, d, k, lo.KN_SLAB_ROWS,
                     idx.data_ptr(), dist.data_ptr(), ws, size, da.stream())
        _sync()
        gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
        if form == "masked":
            wd, wi = kn.masked_topk(X, W, k)
            assert np.array_equal(gi, wi)
            np.testing.assert_allclose(gd, wd, rtol=RTOL, atol=0.0)
        elif form == "manhattan":
            wd, wi = mh.l1_select(mh.l1_distances(X, W), k)
            assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
        else:
            wd, wi = cs.select(cs.cosine_distances(X, W), k)
            assert np.array_equal(gi, wi) and np.array_equal(gd, wd)


# ---- A8. the filtered search: planes, stateless and anchored calls, the run table ---------------------------------------
def _filter_inputs(geom):
    """blobs of float32-valued rows around the prototypes: (X as stored, W)"""
    from tests import anchor_mark as am

    X, W = am.blobs(lo.ROWS, lo.FILTER_D, lo.FILTER_M, ("far", geom))[:2]
    return da.stored(np.asarray(X, dtype=np.float32), lo.dtype_of(geom)), np.ascontiguousarray(W, dtype=np.float64)


def _planes_at(nat, xptr, dtype, N, d, ld):
    total = nat.load().dbgsom_filter_planes_bytes(N, d)
    buf = _full((total + 512,), 0x7f, "uint8")
    bptr = (buf.data_ptr() + 255) // 256 * 256
    nat.call("dbgsom_filter_prepare", xptr, da.CODE[dtype], N, d, ld, bptr, total, da.stream())
    _sync()
    off = bptr - buf.data_ptr()
    return buf, bptr, buf[off:off + total].cpu().numpy()


@pytest.mark.parametrize("geom", lo.PLANES_GEOMS)
def test_filtered_search_far_rows(nat, o, far, geom):
    """the planes and the run table for every storage type and stride (bfloat16 rows 32+ lie past element 2^32); the
    searches for the geometries they take (float32 / float64 rows, 16-byte aligned)"""
    from tests import anchor_mark as am
    from tests import filter_device as fd

    dtype, ld = lo.GEOM[geom]
    N, d, M = lo.ROWS, lo.FILTER_D, lo.FILTER_M
    assert d % 64 == 0
    X, W = _filter_inputs(geom)
    Xw = np.asarray(da.widen(X), dtype=np.float64)
    xptr = far.put(geom, X)
    keep, pptr, host = _planes_at(nat, xptr, dtype, N, d, ld)
    fd.check_prepared(Xw, *fd.split_planes(host, N, d))
    _ct, cptr = da.stage(X, d, 0, dtype)
    assert np.array_equal(host, _planes_at(nat, cptr, dtype, N, d, d)[2])           # the stride changes no bit
    wt, ww = _w_dev(nat, W)
    xx = _norms_at(nat, xptr, dtype, N, d, ld)
    rd, ri = o.bmu_chain(Xw, W, 1)
    wbytes = nat.load().dbgsom_bmu_filtered_workspace_bytes(N, d, M)
    # anchor buckets: four rows of X as anchors, every row with its nearest, bucketed in ascending order of the anchor
    anchors = np.ascontiguousarray(Xw[[0, 9, 18, 34]])
    aof = np.argmin(((Xw[:, None, :] - anchors[None]) ** 2).sum(axis=2), axis=1).astype(np.int32)
    order = np.argsort(aof, kind="stable").astype(np.int32)
    a_t, of_t, or_t = da.dev(anchors), da.dev(aof), da.dev(order)
    for form in ("stateless", "prune", "anchored") if geom in lo.FILTER_GEOMS else ():
        assert lo.aligned16(geom) and dtype in ("f32", "f64")
        ws_t, ws = da.workspace(wbytes)
        idx, dist = _full((N,), -7, "int64"), _full((N,), float("nan"), "float64")
        head = [xptr, da.CODE[dtype], N, d, ld, xx.data_ptr(), pptr, wt.data_ptr(), M, ww.data_ptr()]
        tail = [0, 0, idx.data_ptr(), dist.data_ptr(), ws, wbytes, da.stream()]
        if form == "anchored":
            nat.call("dbgsom_bmu_filtered_anchored", *head, a_t.data_ptr(), len(anchors), of_t.data_ptr(), or_t.data_ptr(),
                     fd.PRUNE, *tail)
        else:
            nat.call("dbgsom_bmu_filtered", *head, None, None, fd.PRUNE if form == "prune" else 0, *tail)
        _sync()
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(dist.cpu().numpy(), rd), form
    # the run table of the buckets
    rbytes = nat.load().dbgsom_anchor_runs_bytes(N, len(anchors))
    rt, rptr = da.workspace(rbytes)
    nat.call("dbgsom_anchor_runs_build", xptr, da.CODE[dtype], N, d, ld, xx.data_ptr(), a_t.data_ptr(), len(anchors),
             of_t.data_ptr(), or_t.data_ptr(), rptr, rbytes, da.stream())
    nb, cap = (N + 127) // 128, (N + 127) // 128 + len(anchors)
    start = np.full(nb + 1, -7, dtype=np.int32)
    ranchor, rR, rxx = np.full(cap, -7, dtype=np.int32), np.full(cap, np.nan), np.full(cap, np.nan)
    nat.call("dbgsom_anchor_runs_read", rptr, N, len(anchors), start.ctypes.data, ranchor.ctypes.data, rR.ctypes.data,
             rxx.ctypes.data, da.stream())
    ref = am.run_table(Xw, anchors, aof, order, xx=xx.cpu().numpy())
    n = int(start[-1])
    assert np.array_equal(start, ref["run_start"]) and np.array_equal(ranchor[:n], ref["anchor"])
    low, high = am.widened_R(ref["R2"], d)
    assert (rR[:n].astype(np.longdouble) >= low).all() and (rR[:n].astype(np.longdouble) <= high).all()
    assert np.array_equal(rxx[:n], ref["xx_max"])


# ---- A9. distortion, exemplars, linear initialisation, sparse codes -------------------------------------------------------
@pytest.mark.parametrize("geom", ["f32-al16", "f32-odd", "f64-odd", "bf16-al16"])
def test_neighborhood_energy_and_exemplars_far_rows(nat, far, geom):
    from tests import distortion as ds
    from tests import exemplars as ex

    dtype, ld = lo.GEOM[geom]
    N, d, M = lo.ROWS, 48 if lo.aligned16(geom) else 33, 33
    X = da.stored(np.asarray(da.widen(lo.random_rows(geom, d, 800 + d, 2.0)), dtype=np.float32), dtype)
    W = _protos(M, d, 83, f32=True)
    xptr = far.put(geom, X)
    wt, ww = _w_dev(nat, W)
    xx = _norms_at(nat, xptr, dtype, N, d, ld)
    R, H = ds.squared_matrix(X, W), ds.gaussian_factors(M)
    hd = da.dev(H)
    size = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, lo.KN_SLAB_ROWS)
    _ws, ws = da.workspace(size)
    bmu, e = _full((N,), ds.BMU_SENTINEL, "int64"), _full((N,), ds.SENTINEL, "float64")
    nat.call("dbgsom_neighborhood_energy", xptr, da.CODE[dtype], N, d, ld, xx.data_ptr(), wt.data_ptr(), M, ww.data_ptr(),
             hd.data_ptr(), M, lo.KN_SLAB_ROWS, bmu.data_ptr(), e.data_ptr(), ws, size, da.stream())
    _sync()
    want_b, want_e = ds.energy_rows(R, H)
    assert np.array_equal(bmu.cpu().numpy(), want_b) and np.array_equal(_bits(e.cpu().numpy()), _bits(want_e))
    for k, own_cell in ((1, 0), (2, 1), (5, 0)):
        size = nat.load().dbgsom_exemplars_workspace_bytes(N, M, k, lo.KN_SLAB_ROWS)
        _ws2, ws2 = da.workspace(size)
        idx, dist = _full((M, k), ex.IDX_SENTINEL, "int64"), _full((M, k), ex.SENTINEL, "float64")
        nat.call("dbgsom_exemplars", xptr, da.CODE[dtype], N, d, ld, xx.data_ptr(), wt.data_ptr(), M, ww.data_ptr(), k,
                 own_cell, lo.KN_SLAB_ROWS, idx.data_ptr(), dist.data_ptr(), ws2, size, da.stream())
        _sync()
        want_d, want_i = ex.exemplars_oracle(R, k, bool(own_cell))
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(_bits(dist.cpu().numpy()), _bits(want_d))


@pytest.mark.parametrize("geom", lo.MASKED_GEOMS)
def test_covariance_apply_far_rows(nat, far, geom):
    from tests import linear_init as li

    dtype, ld = lo.GEOM[geom]
    N, d, p = lo.ROWS, 37, 2
    X = np.array(lo.random_rows(geom, d, 85, 2.0))
    rng = np.random.default_rng(85)
    V = np.ascontiguousarray(rng.normal(size=(d, p)))
    mean = np.asarray(X, dtype=np.float64).sum(axis=0) / N
    Zr, sr, zb, sb = li.exact(X, mean, V)
    size = nat.load().dbgsom_covariance_apply_workspace_bytes(N, d, p)
    _ws, ws = da.workspace(size)
    m_t, v_t = da.dev(mean), da.dev(V)
    _ct, cptr = da.stage(X, d + 3, 0, dtype)
    got = []
    for ptr, ldx in ((far.put(geom, X), ld), (cptr, d + 3)):
        Z, s = _full((d, p), float("nan"), "float64"), _full((d,), float("nan"), "float64")
        nat.call("dbgsom_covariance_apply", ptr, da.CODE[dtype], N, d, ldx, m_t.data_ptr(), v_t.data_ptr(), p, Z.data_ptr(),
                 s.data_ptr(), ws, size, da.stream())
        _sync()
        got.append((Z.cpu().numpy(), s.cpu().numpy()))
    ok_z, worst_z = li.within(got[0][0], Zr, zb)
    ok_s, worst_s = li.within(got[0][1], sr, sb)
    print(f"Z: largest error / bound {worst_z:.3f}, column sums: {worst_s:.3f}")
    assert ok_z and ok_s
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))


@pytest.mark.parametrize("geom", lo.MASKED_GEOMS)
def test_sparse_code_far_rows(nat, far, geom):
    from tests import sparse_code_inputs as si

    dtype, ld = lo.GEOM[geom]
    d, M, C = 24, 12, 3
    W, Xq = si.planted(d, M, 3, lo.ROWS, 0.01, 17)
    X = si.queries(Xq, lo.NP_DTYPE[dtype])
    ref, _iters = si.reference(W, X)
    P = np.random.default_rng(3).random((M, C)) + 0.1
    wt, pt = da.dev(W), da.dev(P)
    size = nat.load().dbgsom_sparse_code_workspace_bytes(lo.ROWS, d, M, 1000)
    _ct, cptr = da.stage(X, d + 1, 0, dtype)
    got = []
    for ptr, ldx in ((far.put(geom, X), ld), (cptr, d + 1)):
        _ws, ws = da.workspace(size)
        code, proba = _full((lo.ROWS, M), float("nan"), "float64"), _full((lo.ROWS, C), float("nan"), "float64")
        counts = _full((len(nat.SC_COUNTS),), 0, "int64")
        nat.call("dbgsom_sparse_code", ptr, da.CODE[dtype], lo.ROWS, d, ldx, wt.data_ptr(), M, d, 1000, 0, pt.data_ptr(), C,
                 code.data_ptr(), proba.data_ptr(), counts.data_ptr(), ws, size, da.stream())
        _sync()
        assert int(counts.cpu()[0]) == lo.ROWS
        got.append((code.cpu().numpy(), proba.cpu().numpy()))
    err = float(np.abs(got[0][0] - ref).max())
    print(f"max |dcode| = {err:.3e}")
    assert err <= si.GATE[np.dtype(lo.NP_DTYPE[dtype])]
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))


# ---- A10. the matrix readers on a far ldr / ldd, the prototype readers on a far ldw, the densified rows -------------------
MATRIX_GEOMS = ["f64-al16", "f64-odd"]


@pytest.mark.parametrize("geom", MATRIX_GEOMS)
def test_matrix_readers_far_rows(nat, far, geom):
    from tests import combined_error as ce
    from tests import distortion as ds
    from tests import exemplars as ex

    _dtype, ldr = lo.GEOM[geom]
    N, M = lo.ROWS, 70
    rng = np.random.default_rng(M)
    R = rng.random((N, M)) * 4.0 + 0.25
    R[5, 11] = R[5, 3]                                  # an equal pair: the lower index first
    rptr = far.put(geom, R)
    for k in (1, 2, 5):
        idx, dist = _full((N, k), kn.IDX_SENTINEL, "int64"), _full((N, k), pd.SENTINEL, "float64")
        nat.call("dbgsom_topk_rows", rptr, N, M, ldr, k, idx.data_ptr(), dist.data_ptr(), da.stream())
        size = nat.load().dbgsom_topk_cols_workspace_bytes(N, M, k)
        _ws, ws = da.workspace(size)
        sr, si_ = _full((M, k), ex.SENTINEL, "float64"), _full((M, k), ex.IDX_SENTINEL, "int64")
        nat.call("dbgsom_topk_cols_init", sr.data_ptr(), si_.data_ptr(), M, k, da.stream())
        nat.call("dbgsom_topk_cols", rptr, N, M, ldr, None, 0, k, sr.data_ptr(), si_.data_ptr(), ws, size, da.stream())
        _sync()
        want_dist, want_idx = kn.topk_lexsort(R, k)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(_bits(dist.cpu().numpy()), _bits(want_dist))
        want_r, want_i = ex.topk_cols_oracle(R, k)
        assert np.array_equal(si_.cpu().numpy(), want_i) and np.array_equal(_bits(sr.cpu().numpy()), _bits(want_r))
    H = ds.gaussian_factors(M)
    hd = da.dev(H)
    bmu, e = _full((N,), ds.BMU_SENTINEL, "int64"), _full((N,), ds.SENTINEL, "float64")
    nat.call("dbgsom_energy_rows", rptr, N, M, ldr, hd.data_ptr(), M, bmu.data_ptr(), e.data_ptr(), da.stream())
    _sync()
    want_b, want_e = ds.energy_rows(R, H)
    assert np.array_equal(bmu.cpu().numpy(), want_b) and np.array_equal(_bits(e.cpu().numpy()), _bits(want_e))
    # dbgsom_combined_error_rows: the distances of the first winners, ldd apart
    idx2 = np.stack([rng.integers(0, M, N), rng.integers(0, M, N)], axis=1).astype(np.int64)
    idx2[7] = (-1, 3)
    D2 = rng.random((N, 2)) * 3.0
    dptr = far.put(geom, D2)
    G = rng.random((M, M)) * 5.0
    gd, id_ = da.dev(G), da.dev(idx2)
    out = _full((N,), ce.SENTINEL, "float64")
    nat.call("dbgsom_combined_error_rows", id_.data_ptr(), dptr, ldr, N, gd.data_ptr(), M, M, out.data_ptr(), da.stream())
    _sync()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ce.combined_error_rows(idx2, D2[:, 0], G)))


@pytest.mark.parametrize("geom", MATRIX_GEOMS)
def test_prototype_readers_far_ldw(nat, far, geom):
    from tests import combined_error as ce

    _dtype, ldw = lo.GEOM[geom]
    M, d = lo.ROWS, 37
    W = _protos(M, d, 87)
    rng = np.random.default_rng(87)
    edges = np.concatenate([rng.integers(0, M, size=(200, 2)), [[0, M - 1], [M - 1, 0], [33, 34], [7, 7]]]).astype(np.int32)
    wptr = far.put(geom, W)
    ed = da.dev(edges)
    out = _full((len(edges),), ce.SENTINEL, "float64")
    nat.call("dbgsom_edge_lengths", wptr, M, d, ldw, ed.data_ptr(), len(edges), out.data_ptr(), da.stream())
    ldwt = nat.load().dbgsom_csr_wt_ld(M)
    Wt = _full((d, ldwt), float("nan"), "float64")
    nat.call("dbgsom_csr_transpose_weights", wptr, M, d, ldw, Wt.data_ptr(), ldwt, da.stream())
    _sync()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ce.edge_lengths(W, edges)))
    want = np.zeros((d, ldwt))
    want[:, :M] = W.T
    assert np.array_equal(_bits(Wt.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("geom", lo.DENSIFY_GEOMS)
def test_csr_densify_into_far_rows(nat, far, geom):
    """the rows are zero-filled over their whole stride (N x ld elements), the stored entries written: the dense matrix
    in the rows, zeros between them, 0xff behind row N - 1"""
    import scipy.sparse as sp

    dtype, ld = lo.GEOM[geom]
    N, d = lo.ROWS, 41
    Xs = sp.random(N, d, density=0.3, format="csr", dtype=lo.NP_DTYPE[dtype], random_state=5)
    Xs.sort_indices()
    far.fill()
    ip, ix, dv = da.dev(Xs.indptr.astype(np.int64)), da.dev(Xs.indices.astype(np.int32)), da.dev(Xs.data)
    nat.call("dbgsom_csr_densify", ip.data_ptr(), ix.data_ptr(), dv.data_ptr(), da.CODE[dtype], N, d, ld, far.base, da.stream())
    _sync()
    rows = far.rows(geom, d)
    assert np.array_equal(rows.cpu().numpy(), Xs.toarray())
    rows.zero_()
    end = N * lo.row_bytes(geom)
    assert end % 8 == 0
    step = 2 ** 27
    for a in range(0, end // 8, step):
        assert not bool(far.words[a:min(a + step, end // 8)].any()), "a stray write between the rows"
    assert bool((far.words[end // 8:] == -1).all()), "a write behind row N - 1"


# =========================================================================================================================
# Part B: tall compact rows
# =========================================================================================================================
class Tall:
    """the two tall matrices, one at a time: T32 (float32, d = 1024) and T16 (bfloat16, d = 2048), blobs generated on
    the device by bench.make_shard"""

    def __init__(self):
        self.name, self.X = None, None

    def get(self, which):
        import torch

        import bench

        if self.name == which:
            return self.X
        self.drop()
        dtype, N, d = lo.T32 if which == "T32" else lo.T16
        _need(lo.PEAK_BYTES)
        if dtype == "f32":
            X = bench.make_shard(torch, N, d, 7, "cuda")
        else:       # (the same centres for every piece, the rows of piece r from the stream of rank r)
            X = torch.empty((N, d), dtype=torch.bfloat16, device="cuda")
            step = 2 ** 18
            for r, s in enumerate(range(0, N, step)):
                m = min(step, N - s)
                X[s:s + m] = bench.make_shard(torch, m, d, 7, "cuda", rank=r).to(torch.bfloat16)
        assert X.is_contiguous() and X.data_ptr() % 256 == 0 and X.numel() == N * d
        self.name, self.X = which, X
        return X

    def drop(self):
        import torch

        self.name, self.X = None, None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tall():
    t = Tall()
    yield t
    t.drop()


def _rows_f64(X, rows):
    """rows of a device matrix, widened exactly, on the host"""
    import torch

    return X[torch.from_numpy(rows).cuda()].double().cpu().numpy()


def _map_from(X, M, seed):
    """M prototypes: rows of X (the last one among them) moved a little, float64 and not float32-valued"""
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(X.shape[0] - 1, M - 1, replace=False))
    W = _rows_f64(X, np.concatenate([rows, [X.shape[0] - 1]]).astype(np.int64))
    return np.ascontiguousarray(W + 0.01 * rng.normal(size=W.shape))


@pytest.fixture(scope="module")
def epoch32(tall, o):
    """one epoch of T32 under both searches at M = 64 (8 x 8) and M = 144 (12 x 12: the filtered search takes maps of
    129 prototypes and more, SearchPolicy::FILTER_MIN_PROTOTYPES), everything they returned, and the picked rows:
    {M: {W, hop, filtered, exact, filtered_log, exact_log}, rows, Xp}"""
    from dbgsom_amd.backend import HipBackend
    from tests import golden_inputs as gi

    X = tall.get("T32")
    _dt, N, d = lo.T32
    out = {"sigma": 1.6, "gamma": 1e-4}
    for side in lo.TALL_SIDES:
        M = side * side
        e = {"W": _map_from(X, M, side), "hop": gi.lattice_hops(side, side)}
        for alg in ("filtered", "exact"):
            be = HipBackend(0, algorithm=alg)
            try:
                be.load_device(X)
                e[alg] = be.epoch(e["W"], e["hop"], out["sigma"], out["gamma"], want_assignments=True)
                e[alg + "_log"] = list(be.filter_log)
            finally:
                be.release()
                del be
        out[M] = e
    rows = lo.picked_rows("f32", N, d)
    out["rows"], out["Xp"] = rows, _rows_f64(X, rows)
    return out


# ---- B1. the epoch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", lo.TALL_SIDES)
def test_tall_epoch_filtered_equals_exact_and_the_oracle(epoch32, o, side):
    """M = 64 is below the smallest map the filtered search takes: both contexts run the all-pairs search there, and the
    log says so.  At M = 144 the filtered path runs."""
    _dt, N, d = lo.T32
    M = side * side
    e = epoch32[M]
    fi, ex = e["filtered"], e["exact"]
    assert e["filtered_log"] and not e["exact_log"]
    assert e["filtered_log"][-1][0] == ("filtered" if M >= lo.FILTER_MIN_M else "exact")
    assert np.array_equal(fi.winners, ex.winners) and np.array_equal(_bits(fi.distances), _bits(ex.distances))
    assert np.array_equal(_bits(fi.new_weights), _bits(ex.new_weights))
    assert np.array_equal(_bits(fi.errors), _bits(ex.errors)) and fi.change_total == ex.change_total
    assert np.array_equal(fi.activations, ex.activations) and fi.activations.sum() == N
    assert np.array_equal(fi.activations, np.bincount(fi.winners, minlength=M))
    rows = epoch32["rows"]
    assert rows[-1] == N - 1 and (rows * d >= 2 ** 31).any() and (rows * d * 4 >= 2 ** 32).any()
    rd, ri = o.bmu_chain(epoch32["Xp"], e["W"], 1)
    assert np.array_equal(fi.winners[rows], ri) and np.array_equal(_bits(fi.distances[rows]), _bits(rd))
    assert not np.isnan(fi.new_weights).any()


# ---- B7. node statistics and quantization error (while the epoch's matrix is resident) ----------------------------------------
def test_tall_node_statistics_and_quantization_error(tall, epoch32):
    import math

    from dbgsom_amd.backend import HipBackend

    X = tall.get("T32")
    e = epoch32[lo.TALL_M]
    W, win, dist = e["W"], e["exact"].winners, e["exact"].distances
    M = lo.TALL_M
    be = HipBackend(0)
    try:
        be.load_device(X)
        qe = be.quantization_error(W)
        sigma = 1.7
        hits, dens = be.node_statistics(W, sigma)
    finally:
        be.release()
    np.testing.assert_allclose(qe, math.fsum(dist) / len(dist), rtol=1e-12)
    assert np.array_equal(hits, np.bincount(win, minlength=M))
    terms = np.exp(-(dist ** 2) / (2 * sigma ** 2)) / (sigma * np.sqrt(2 * np.pi))
    np.testing.assert_allclose(dens, np.bincount(win, weights=terms, minlength=M), rtol=1e-12, atol=1e-300)


# ---- B2. the per-neuron sums -------------------------------------------------------------------------------------------------
def _segment_reference(X, win_t, f_t, M, chunk=50000):
    """float64 sums S_j = sum f_i x_i and T_j = sum |f_i x_i| over the rows with winner j (winners outside [0, M) skipped),
    torch.index_add_ over `chunk` rows at a time"""
    import torch

    N, d = X.shape
    S = torch.zeros((M, d), dtype=torch.float64, device="cuda")
    T = torch.zeros_like(S)
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        w = win_t[s:e]
        ok = (w >= 0) & (w < M)
        terms = f_t[s:e, None] * X[s:e].double()
        S.index_add_(0, w[ok], terms[ok])
        T.index_add_(0, w[ok], terms[ok].abs())
    return S.cpu().numpy(), T.cpu().numpy()


def _tall_winners(N, M, seed):
    """neuron 1 empty, neuron M - 1 owns rows among the last 4096 only"""
    rng = np.random.default_rng(seed)
    pool = np.array([j for j in range(M - 1) if j != 1])
    win = pool[rng.integers(0, len(pool), N)].astype(np.int64)
    win[N - 4096 + rng.choice(4096, 1000, replace=False)] = M - 1
    win[N - 1] = M - 1
    return win


def _check_tall_sums(nat, X, dtype, weighted):
    import torch

    N, d = X.shape
    M = lo.TALL_M
    win = _tall_winners(N, M, d)
    gen = torch.Generator(device="cuda").manual_seed(d)
    kw_t = 1.0 - torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
    dist_t = 3.0 * torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
    sw_t = torch.randint(0, 4, (N,), device="cuda", generator=gen).double() if weighted else None
    if weighted:
        sw_t[N - 1] = 2.0
    win_t = da.dev(win)
    name = "dbgsom_accumulate_weighted" if weighted else "dbgsom_accumulate"
    nbytes = getattr(nat.load(), name + "_workspace_bytes")(N, d, M)
    ws_t, ws = da.workspace(nbytes)
    u_lead = 2 if weighted else 1                    # (weighted: one more rounding per row, the factor sw kw)

    def call(winners_t):
        sums = _full((M * (d + 3),), float("nan"), "float64")
        st = _full((1,), 77, "int32")
        args = [X.data_ptr(), da.CODE[dtype], N, d, d, winners_t.data_ptr(), kw_t.data_ptr()]
        if weighted:
            args.append(sw_t.data_ptr())
        args += [dist_t.data_ptr(), M, sums.data_ptr(), st.data_ptr(), ws, nbytes, da.stream()]
        nat.call(name, *args)
        _sync()
        v = sums.cpu().numpy()
        return v[:M * d].reshape(M, d), v[M * d:M * d + M], v[M * d + M:M * d + 2 * M], v[M * d + 2 * M:], int(st.cpu()[0])

    def check(winners, winners_t, S, K, a, E):
        inside = (winners >= 0) & (winners < M)
        n = np.bincount(winners[inside], minlength=M)
        f_t = sw_t * kw_t if weighted else kw_t
        e_t = sw_t * dist_t if weighted else dist_t
        Sr, TS = _segment_reference(X, winners_t, f_t, M)
        ones = torch.ones((N, 1), dtype=torch.float64, device="cuda")
        Kr, TK = (v[:, 0] for v in _segment_reference(ones, winners_t, f_t, M))
        Er, TE = (v[:, 0] for v in _segment_reference(ones, winners_t, e_t, M))
        if weighted:
            assert np.array_equal(a, np.bincount(winners[inside], weights=sw_t.cpu().numpy()[inside], minlength=M))
        else:
            assert np.array_equal(a, n) and a.sum() == inside.sum()
        for label, got, ref, T, nn in (("S", S, Sr, TS, n[:, None]), ("K", K, Kr, TK, n), ("E", E, Er, TE, n)):
            bound = 2.0 * u_lead * (nn + 2) * da.U * T
            err = np.abs(got - ref)
            worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
            print(f"{label}: largest error / bound {worst:.3f}")
            assert np.all(err <= bound), label
        assert not n[1] and (S[1] == 0).all() and K[1] == 0 and E[1] == 0 and a[1] == 0
        return n

    S, K, a, E, st = call(win_t)
    assert st == 0 and not any(np.isnan(p).any() for p in (S, K, a, E))
    n = check(win, win_t, S, K, a, E)
    assert n[M - 1] == np.count_nonzero(win[N - 4096:] == M - 1) > 0
    skip = ws - ws_t.data_ptr()
    order = ws_t[skip:skip + 4 * N].cpu().numpy().view(np.int32)
    assert np.array_equal(order, np.argsort(win, kind="stable"))
    # a winner outside the map in the last row: the status is set and that row is skipped
    bad = win.copy()
    bad[N - 1] = M
    bad_t = da.dev(bad)
    S2, K2, a2, E2, st2 = call(bad_t)
    assert st2 != 0
    check(bad, bad_t, S2, K2, a2, E2)
    assert a2[M - 1] == a[M - 1] - (2.0 if weighted else 1.0)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_tall_sums_float32(nat, tall, weighted):
    _check_tall_sums(nat, tall.get("T32"), "f32", weighted)


# ---- B3. the bucket sort ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["modulo", "skewed"])
def test_tall_bucket_sort_is_the_stable_order(nat, kind):
    from tests import epoch_tail as et

    N, M, d = lo.TALL_N, 1024, et.SORT_D
    win = et.sort_winners(kind, N, M)
    assert win.min() >= 0 and win.max() < M
    X = _full((N, d), 1.0, "float32")
    win_t, one = da.dev(win), _full((N,), 1.0, "float64")
    nbytes = nat.load().dbgsom_accumulate_workspace_bytes(N, d, M)
    ws_t, ws = da.workspace(nbytes)
    sums, st = _full((M * (d + 3),), float("nan"), "float64"), _full((1,), 77, "int32")
    nat.call("dbgsom_accumulate", X.data_ptr(), da.F32, N, d, d, win_t.data_ptr(), one.data_ptr(), one.data_ptr(), M,
             sums.data_ptr(), st.data_ptr(), ws, nbytes, da.stream())
    _sync()
    skip = ws - ws_t.data_ptr()
    order = ws_t[skip:skip + 4 * N].cpu().numpy().view(np.int32)
    assert np.array_equal(order, np.argsort(win, kind="stable"))
    v = sums.cpu().numpy()
    counts = np.bincount(win, minlength=M)
    assert int(st.cpu()[0]) == 0 and np.array_equal(v[M * d + M:M * d + 2 * M], counts)
    assert np.array_equal(v[:M * d].reshape(M, d), np.repeat(counts[:, None], d, axis=1))       # (sums of ones: exact)


# ---- B4. column moments -------------------------------------------------------------------------------------------------------
def _column_chains(X, mean):
    """the chains of dbgsom_ctx_column_sums on the host, bit for bit: per column acc = acc + x_i and, with the float32
    mean, y = x_i - m; y = y * y; acc = acc + y, each operation rounded on its own, i ascending.  The rows come down in
    pieces into a page-locked buffer whose first row carries the running sums (NumPy reduces axis 0 row after row);
    the columns are independent, so blocks of them go to threads."""
    import torch
    from concurrent.futures import ThreadPoolExecutor

    N, d = X.shape
    step, nthr = 2 ** 16, 8
    pin = torch.empty((step + 1, d), dtype=torch.float32).pin_memory()
    buf = pin.numpy()
    sq = np.empty_like(buf)
    acc1, acc2 = np.zeros(d, dtype=np.float32), np.zeros(d, dtype=np.float32)
    edges = np.linspace(0, d, nthr + 1).astype(int)

    def block(args):
        lo_, hi, m = args
        buf[0, lo_:hi] = acc1[lo_:hi]
        sq[0, lo_:hi] = acc2[lo_:hi]
        np.subtract(buf[1:m + 1, lo_:hi], mean[lo_:hi], out=sq[1:m + 1, lo_:hi])
        np.multiply(sq[1:m + 1, lo_:hi], sq[1:m + 1, lo_:hi], out=sq[1:m + 1, lo_:hi])
        acc1[lo_:hi] = np.add.reduce(buf[:m + 1, lo_:hi], axis=0)
        acc2[lo_:hi] = np.add.reduce(sq[:m + 1, lo_:hi], axis=0)

    with ThreadPoolExecutor(nthr) as pool:
        for s0 in range(0, N, step):
            m = min(step, N - s0)
            pin[1:m + 1].copy_(X[s0:s0 + m])
            list(pool.map(block, [(edges[t], edges[t + 1], m) for t in range(nthr)]))
    return acc1, acc2


def test_column_chains_helper_is_the_row_by_row_loop():
    """(the helper above against tests/device_abi.column_sums_loop on a matrix small enough for the loop)"""
    import torch

    rng = np.random.default_rng(12)
    A = (rng.normal(size=(1000, 24)) * 2.0 + 0.5).astype(np.float32)
    mean = (da.column_sums_loop(A) / np.float32(1000)).astype(np.float32)
    s1, s2 = _column_chains(torch.from_numpy(A).cuda(), mean)
    assert np.array_equal(s1, da.column_sums_loop(A)) and np.array_equal(s2, da.column_sums_loop(A, mean))


def test_tall_column_moments(tall, epoch32):
    """dbgsom_ctx_column_sums: the float32 chains bit for bit (_column_chains).  dbgsom_ctx_weighted_column_sums twice:
    with a weight on every row against chunked float64 sums, within (N + 2) u sum |terms| for the kernel (the bound of
    tests/test_gpu_device_abi.py) plus as much for the reference's own error (float64 sums of the same terms in another
    order); and with every weight 0 but the picked rows', whose sums np.longdouble gives within (n + 2) u sum |terms|.
    dbgsom_ctx_covariance_apply: the bounds of tests/linear_init.py for the kernel plus as much for the chunked float64
    reference (li.exact is np.longdouble on the host and takes the whole matrix)."""
    import torch

    from dbgsom_amd.backend import HipBackend
    from tests import linear_init as li

    X = tall.get("T32")
    N, d = X.shape
    rows, Xp = epoch32["rows"], epoch32["Xp"]
    rng = np.random.default_rng(4)
    w = np.zeros(N)
    w[rows] = rng.integers(1, 4, len(rows)) * rng.uniform(0.1, 2.5, len(rows))
    w_all = rng.integers(1, 4, N) * rng.uniform(0.1, 2.5, N)
    V = np.ascontiguousarray(rng.normal(size=(d, 2)))
    be = HipBackend(0)
    try:
        be.load_device(X)
        s1, s2, n = be.column_moments()
        mean64 = np.asarray(s1, dtype=np.float64) / N
        Z, colsum = be.covariance_apply(mean64, V)
        be.set_sample_weight(w)
        total = be.weight_total()
        ws1, ws2 = be.weighted_column_moments(total)
        be.set_sample_weight(w_all)
        total_all = be.weight_total()
        wa1, wa2 = be.weighted_column_moments(total_all)
    finally:
        be.release()
    assert n == N and s1.dtype == np.float32
    c1, c2 = _column_chains(X, np.ascontiguousarray(np.true_divide(s1, N)))
    assert np.array_equal(s1, c1) and np.array_equal(s2, c2)
    m64, v_t, w_t = torch.from_numpy(mean64).cuda(), torch.from_numpy(V).cuda(), torch.from_numpy(w_all).cuda()
    mw = torch.from_numpy(np.ascontiguousarray(wa1 / total_all)).cuda()
    zero = torch.zeros(d, dtype=torch.float64, device="cuda")
    zr, zb, sr, sb = torch.zeros_like(v_t), torch.zeros_like(v_t), zero.clone(), zero.clone()
    r1, t1, r2 = zero.clone(), zero.clone(), zero.clone()
    for s in range(0, N, 50000):
        c = X[s:s + 50000].double()
        wc = w_t[s:s + 50000, None]
        r1 += (wc * c).sum(dim=0)
        t1 += (wc * c).abs().sum(dim=0)
        r2 += (wc * (c - mw) ** 2).sum(dim=0)
        c -= m64
        zr += c.T @ (c @ v_t)
        sr += c.sum(dim=0)
        c.abs_()
        zb += c.T @ (c @ v_t.abs())
        sb += c.sum(dim=0)
    L = np.longdouble
    for label, got, ref, T in (("w x", wa1, r1, t1), ("w (x - m)^2", wa2, r2, r2)):
        ref, T = ref.cpu().numpy(), T.cpu().numpy()
        bound = 2 * (N + 2) * da.U * T
        err = np.abs(got - ref)
        print(f"weighted column sums, {label}: largest error / bound {float(np.max(err / bound)):.4f}")
        assert np.all(err <= bound), label
    assert abs(total_all - math_fsum(w_all)) <= (N + 2) * da.U * math_fsum(w_all)
    ok_z, worst_z = li.within(Z, zr.cpu().numpy().astype(L), 2 * (N + d + 8) * li.U * zb.cpu().numpy().astype(L))
    ok_s, worst_s = li.within(colsum, sr.cpu().numpy().astype(L), 2 * (N + 8) * li.U * sb.cpu().numpy().astype(L))
    print(f"covariance_apply: Z error / bound {worst_z:.3f}, column sums {worst_s:.3f}")
    assert ok_z and ok_s
    # the weighted sums of the picked rows alone
    wl = w[rows].astype(L)
    assert abs(L(total) - wl.sum()) <= (len(rows) + 2) * da.U * wl.sum()
    m = ws1 / total
    for got, base in ((ws1, Xp.astype(L)), (ws2, (Xp.astype(L) - m.astype(L)) ** 2)):
        terms = wl[:, None] * base
        ref, T = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        bound = (len(rows) + 2) * da.U * T + 2 * len(rows) * da.UL * T
        assert np.all(np.abs(got.astype(L) - ref) <= bound)


# ---- B5. queries -----------------------------------------------------------------------------------------------------------------
def test_tall_queries(nat, o, tall, epoch32):
    import torch

    from dbgsom_amd.backend import HipBackend

    X = tall.get("T32")
    N, d = X.shape
    M = lo.QUERY_M
    rows, Xp = epoch32["rows"], epoch32["Xp"]
    W = _map_from(X, M, 2)
    rd, ri = o.bmu_chain(Xp, W, 1)
    pick_t = torch.from_numpy(rows).cuda()
    be = HipBackend(0)
    try:
        dist_t, idx_t = be.bmu(W, 1, X=X)                       # dbgsom_ctx_bmu_query_device on all of the rows
        assert isinstance(idx_t, torch.Tensor) and idx_t.shape[0] == N
        assert np.array_equal(idx_t[pick_t].cpu().numpy().reshape(-1), ri)
        assert np.array_equal(_bits(dist_t[pick_t].cpu().numpy().reshape(-1)), _bits(rd))
        assert int(idx_t.min()) >= 0 and int(idx_t.max()) < M
        del dist_t, idx_t
    finally:
        be.release()
    # the raw matrix: N x M float64, 5.05e9 bytes
    wt, ww = _w_dev(nat, W)
    xx = _norms_at(nat, X.data_ptr(), "f32", N, d, d)
    D = _full((N, M), pd.SENTINEL, "float64")
    assert D.numel() * 8 > 2 ** 32
    nat.call("dbgsom_distances", X.data_ptr(), da.F32, N, d, d, xx.data_ptr(), wt.data_ptr(), M, ww.data_ptr(), D.data_ptr(),
             M, da.stream())
    _sync()
    want = pd.pair_distances(Xp, W)
    assert np.array_equal(_bits(D[pick_t].cpu().numpy()), _bits(want))
    assert rows[-1] == N - 1 and np.array_equal(_bits(D[N - 1].cpu().numpy()), _bits(want[-1]))
    assert not bool((D == pd.SENTINEL).any())
    del D
    torch.cuda.empty_cache()
    k = 5
    size = nat.load().dbgsom_kneighbors_workspace_bytes(N, M, 0)
    _ws, ws = da.workspace(size)
    idx, dist = _full((N, k), kn.IDX_SENTINEL, "int64"), _full((N, k), pd.SENTINEL, "float64")
    nat.call("dbgsom_kneighbors", X.data_ptr(), da.F32, N, d, d, xx.data_ptr(), wt.data_ptr(), M, ww.data_ptr(), k, 0,
             idx.data_ptr(), dist.data_ptr(), ws, size, da.stream())
    _sync()
    wi = kn.topk_oracle(Xp, W, k, want)
    assert np.array_equal(idx[pick_t].cpu().numpy(), wi)
    assert np.array_equal(_bits(dist[pick_t].cpu().numpy()), _bits(np.take_along_axis(want, wi, axis=1)))


# ---- B6. vertical growth: partition, subset, labels and weights -------------------------------------------------------------------
def test_tall_partition_and_subset(tall, epoch32):
    import torch

    from dbgsom_amd.backend import HipBackend

    X = tall.get("T32")
    N, d = X.shape
    W, win = epoch32[lo.TALL_M]["W"], epoch32[lo.TALL_M]["exact"].winners
    M, C = lo.TALL_M, 5
    rng = np.random.default_rng(6)
    y = rng.integers(0, C, N).astype(np.int32)
    w = rng.integers(0, 4, N).astype(np.float64)
    j = int(win[N - 1])                                          # the neuron that owns the last row
    members = np.flatnonzero(win == j)
    be = HipBackend(0, algorithm="exact")
    child = None
    try:
        be.load_device(X)
        be.set_labels(y)
        be.set_sample_weight(w)
        counts, got_win = be.partition(W, want_winners=True)
        assert np.array_equal(got_win, win) and np.array_equal(counts, np.bincount(win, minlength=M))
        child = be.subset(j)
        assert child.n_samples == len(members) and members[-1] == N - 1
        for a in range(0, len(members), 8192):                   # every row of the child, in order
            take = np.arange(a, min(a + 8192, len(members)))
            assert np.array_equal(child.read_samples(take), _rows_f64(X, members[take])), a
        assert child.weight_total() == w[members].sum()          # (small integers: exact)
        hist = child.class_histogram(np.zeros(len(members), dtype=np.int64), C, 1)
        assert np.array_equal(np.asarray(hist).reshape(-1), np.bincount(y[members], weights=w[members], minlength=C))
    finally:
        if child is not None:
            child.release()
        be.release()


# ---- B2 again, on the bfloat16 matrix (T32 is released first) --------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_tall_sums_bfloat16(nat, tall, weighted):
    X = tall.get("T16")
    assert X.numel() > 2 ** 32
    _check_tall_sums(nat, X, "bf16", weighted)


def test_tall_bfloat16_through_the_context(tall, o):
    """the engine's own paths on the matrix with more than 2^32 elements: the search, the bucket order and the gathers"""
    from dbgsom_amd.backend import HipBackend

    X = tall.get("T16")
    _dt, N, d = lo.T16
    M = lo.TALL_M
    W = _map_from(X, M, 16)
    rows = lo.picked_rows("bf16", N, d)
    assert (rows * d >= 2 ** 32).any() and (rows * d < 2 ** 32).any() and rows[-1] == N - 1
    Xp = _rows_f64(X, rows)
    rd, ri = o.bmu_chain(Xp, W, 1)
    be = HipBackend(0, algorithm="exact")
    child = None
    try:
        be.load_device(X)
        assert np.array_equal(be.read_samples(rows), Xp)
        counts, win = be.partition(W, want_winners=True)
        assert np.array_equal(win[rows], ri) and np.array_equal(counts, np.bincount(win, minlength=M))
        j = int(win[N - 1])
        members = np.flatnonzero(win == j)
        child = be.subset(j)
        assert child.n_samples == len(members)
        take = np.arange(max(0, len(members) - 4096), len(members))
        assert np.array_equal(child.read_samples(take), _rows_f64(X, members[take]))
    finally:
        if child is not None:
            child.release()
        be.release()


def test_peak_memory_stays_inside_the_stated_need(tall):
    import torch

    tall.drop()
    peak = torch.cuda.max_memory_allocated()
    print(f"large-offset module: {time.monotonic() - T0:.1f} s wall, peak device memory {peak / 1e9:.2f} GB")
    assert peak <= lo.TOTAL + lo.PEAK_BYTES          # (what the fixtures ask the card for before they allocate)
