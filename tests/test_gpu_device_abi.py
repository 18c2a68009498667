"""MI355X: the device-level entry points of include/dbgsom_hip.h called the way the header allows and the context
never does -- any d >= 1, a row stride ld > d, a base that is not 16-byte aligned, crafted winner lists -- against
plain NumPy references (tests/device_abi.py).  Padding columns hold NaN: a read of them poisons the result.
The chains (row norms, BMU search) are compared bit for bit with oracle/, the ordered sums within
(n + 2) u sum |terms| of the exact sums, integer results exactly."""
from fractions import Fraction

import numpy as np
import pytest

from tests import device_abi as da
from tests.device_abi import U

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


def _empty(shape, dtype):
    import torch

    return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")


def _full(shape, value, dtype):
    import torch

    return torch.full(shape, value, dtype=getattr(torch, dtype), device="cuda")


def _norms_dev(nat, A, ld, off, dtype):
    """dbgsom_row_sqnorms on the staged rows of A -> device tensor (the caller synchronises)"""
    t, ptr = da.stage(A, ld, off, dtype)
    out = _full((A.shape[0],), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", ptr, da.CODE[dtype], A.shape[0], A.shape[1], ld, out.data_ptr(), da.stream())
    return out, t


# ---- 1. dbgsom_row_sqnorms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rows,d,ld", da.NORM_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_row_sqnorms_strided_and_unaligned(nat, o, dtype, rows, d, ld, off):
    rng = np.random.default_rng(rows + d + ld)
    A = da.stored(rng.normal(size=(rows, d)) * rng.uniform(0.5, 3.0, size=d), dtype)
    out, _keep = _norms_dev(nat, A, ld, off, dtype)
    _sync()
    assert np.array_equal(out.cpu().numpy(), o.row_sqnorms_chain(da.widen(A)))


# ---- 2. dbgsom_bmu --------------------------------------------------------------------------------------------------
def _bmu_call(nat, o, dtype, X, W, ldx, x_off, w_off, k, round_f32):
    """dbgsom_bmu with xx / ww from dbgsom_row_sqnorms on the same rows; W contiguous, w_off elements into its
    allocation -> (dist, idx) shaped as o.bmu_chain returns them"""
    N, d = X.shape
    M = W.shape[0]
    xx, xt = _norms_dev(nat, X, ldx, x_off, dtype)
    xptr = xt.data_ptr() + x_off * da.ITEM[dtype]
    ww, wt = _norms_dev(nat, W, d, w_off, "f64")
    wptr = wt.data_ptr() + w_off * 8
    idx = _full((N, k), -7, "int64")
    dist = _full((N, k), float("nan"), "float64")
    nat.call("dbgsom_bmu", xptr, da.CODE[dtype], N, d, ldx, xx.data_ptr(), wptr, M, ww.data_ptr(), k, round_f32,
             idx.data_ptr(), dist.data_ptr(), da.stream())
    _sync()
    assert np.array_equal(xx.cpu().numpy(), o.row_sqnorms_chain(da.widen(X)))
    assert np.array_equal(ww.cpu().numpy(), o.row_sqnorms_chain(W))
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    if k == 1:
        dist, idx = dist.reshape(-1), idx.reshape(-1)
    return dist, idx


def _bmu_data(dtype, N, d, M, seed, round_f32=0):
    rng = np.random.default_rng(seed)
    X = da.stored(rng.normal(size=(N, d)) * rng.uniform(0.5, 3.0, size=d), dtype)
    W = rng.normal(size=(M, d)) * 1.5
    if round_f32:
        W = W.astype(np.float32).astype(np.float64)     # float32 prototypes, as in epoch 0 of a float32 fit
    return X, W


@pytest.mark.parametrize("dtype,N,d,M,pad,x_off,w_off,k,round_f32", da.BMU_CASES)
def test_bmu_register_staged_kernel_unpadded(nat, o, dtype, N, d, M, pad, x_off, w_off, k, round_f32):
    assert da.bmu_class(dtype, d, d + pad, x_off, 8 * w_off, M)[0] == "reg"
    X, W = _bmu_data(dtype, N, d, M, 31 * N + d + M, round_f32)
    dist, idx = _bmu_call(nat, o, dtype, X, W, d + pad, x_off, w_off, k, round_f32)
    rd, ri = o.bmu_chain(da.widen(X), W.astype(np.float32) if round_f32 else W, k)
    assert np.array_equal(idx, ri)
    assert np.array_equal(dist, rd)
    if round_f32:
        assert np.array_equal(dist, dist.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("dtype,N,d,M,ldx", da.BMU_DMA_CASES)
def test_bmu_dma_kernel_with_strided_rows(nat, o, dtype, N, d, M, ldx):
    assert da.bmu_class(dtype, d, ldx, 0, 0, M)[0] == "dma"
    X, W = _bmu_data(dtype, N, d, M, N + M + ldx)
    for k in (1, 2):
        dist, idx = _bmu_call(nat, o, dtype, X, W, ldx, 0, 0, k, 0)
        rd, ri = o.bmu_chain(X, W, k)
        assert np.array_equal(idx, ri) and np.array_equal(dist, rd)


def test_bmu_ties_to_the_lowest_index_unpadded(nat, o):
    """the duplicated-prototype block of test_ties_lowest_index at d = 12 as it is (the context pads it to 16)"""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 5, size=(6, 12)).astype(np.float64)
    W = np.tile(base, (60, 1))
    X = rng.integers(0, 5, size=(500, 12)).astype(np.float64)
    assert da.bmu_class("f64", 12, 12, 0, 0, 360) == ("reg", 1, 1)
    dist, idx = _bmu_call(nat, o, "f64", X, W, 12, 0, 0, 2, 0)
    assert (idx[:, 0] < 6).all()
    rd, ri = o.bmu_chain(X, W, 2)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    assert (dist[:, 0] == dist[:, 1]).all() and (idx[:, 1] > idx[:, 0]).all()


# ---- 3. dbgsom_accumulate / dbgsom_accumulate_weighted ------------------------------------------------------------
def _accumulate_call(nat, dtype, X, ldx, off, winners, kw, dist, M, sw=None, status=True):
    """-> (sums as (S, K, a, E), status word or None, the first N int32 of the workspace), called twice: the second
    call's bits must be the first's"""
    lib = nat.load()
    N, d = X.shape
    xt, xptr = da.stage(X, ldx, off, dtype)
    win_t, kw_t, dist_t = da.dev(winners), da.dev(kw), da.dev(dist)
    sw_t = da.dev(sw) if sw is not None else None
    name = "dbgsom_accumulate_weighted" if sw is not None else "dbgsom_accumulate"
    nbytes = getattr(lib, name + "_workspace_bytes")(N, d, M)
    assert nbytes > 0
    ws_t, ws = da.workspace(nbytes)
    outs = []
    for _ in range(2):
        sums = _full((M * (d + 3),), float("nan"), "float64")
        st = _full((1,), 77, "int32") if status else None
        args = [xptr, da.CODE[dtype], N, d, ldx, win_t.data_ptr(), kw_t.data_ptr()]
        if sw is not None:
            args.append(sw_t.data_ptr())
        args += [dist_t.data_ptr(), M, sums.data_ptr(), st.data_ptr() if status else None, ws, nbytes, da.stream()]
        nat.call(name, *args)
        _sync()
        outs.append((sums.cpu().numpy(), int(st.cpu()[0]) if status else None))
    assert np.array_equal(outs[0][0], outs[1][0], equal_nan=True) and outs[0][1] == outs[1][1]   # the same bits twice
    v = outs[0][0]
    skip = (ws - ws_t.data_ptr())
    order = ws_t[skip:skip + 4 * N].cpu().numpy().view(np.int32)
    return (v[:M * d].reshape(M, d), v[M * d:M * d + M], v[M * d + M:M * d + 2 * M], v[M * d + 2 * M:]), outs[0][1], order


def _check_accumulate(nat, case, status=True):
    dtype, X, ldx, off, winners, kw, dist, M, sw, integer_weights = case
    (S, K, a, E), st, order = _accumulate_call(nat, dtype, X, ldx, off, winners, kw, dist, M, sw, status)
    inside = (winners >= 0) & (winners < M)
    (Sr, Kr, ar, Er), (TS, TK, TE) = da.accumulate_reference(da.widen(X), winners, kw, dist, M, sw)
    n = np.bincount(winners[inside], minlength=M)
    assert not np.isnan(S).any() and not np.isnan(K).any() and not np.isnan(a).any() and not np.isnan(E).any()
    if sw is None:
        assert np.array_equal(a, n) and a.sum() == inside.sum()                 # no row is left out
    elif integer_weights:
        assert np.array_equal(a, np.bincount(winners[inside], weights=sw[inside], minlength=M))
    else:
        ar_, Ta = da.segment_sums(sw[inside], winners[inside], M)
        ok, r = da.sums_within_bound(a, ar_, Ta, n, False)
        print(f"a: largest error / bound {r:.3f}")
        assert ok
    for name, got, ref, T in (("S", S, Sr, TS), ("K", K, Kr, TK), ("E", E, Er, TE)):
        ok, r = da.sums_within_bound(got, ref, T, n, sw is not None)
        print(f"{name}: largest error / bound {r:.3f}")
        assert ok, name
    empty = n == 0
    assert (S[empty] == 0).all() and (K[empty] == 0).all() and (E[empty] == 0).all() and (a[empty] == 0).all()
    if status:
        assert (st != 0) == (not inside.all())
    if inside.all():
        assert np.array_equal(order, np.argsort(winners, kind="stable"))       # the header's contract for order_dev


@pytest.mark.parametrize("dtype,d,pad,off,weighted", da.SEGSUM_CASES)
def test_accumulate_every_segsum_instantiation(nat, dtype, d, pad, off, weighted):
    _check_accumulate(nat, da.segsum_case(dtype, d, pad, off, weighted))


@pytest.mark.parametrize("weights", [None, "int", "frac"])
def test_accumulate_list_lengths_around_the_chunk_size(nat, weights):
    _check_accumulate(nat, da.list_case(weights))


@pytest.mark.parametrize("M", sorted(da.GROUP_CASES))
@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_second_level_sum(nat, M, weighted):
    _check_accumulate(nat, da.group_case(M, weighted))


def test_accumulate_largest_lds_histogram(nat):
    _check_accumulate(nat, da.histogram_case())


@pytest.mark.parametrize("N", da.SCATTER_N)
def test_accumulate_both_scatter_kernels(nat, N):
    _check_accumulate(nat, da.scatter_case(N))


@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_status_and_skipped_rows(nat, weighted):
    for bad in (False, True):              # in range: status 0; one -1 and one M: status set, the two rows skipped
        for status in (True, False):       # (False: status_dev = NULL)
            _check_accumulate(nat, da.status_case(weighted, bad), status)


@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_of_no_rows_returns_zeros(nat, weighted):
    M, d = 7, 5
    sums = _full((M * (d + 3),), float("nan"), "float64")
    st = _full((1,), 77, "int32")
    ws_t, ws = da.workspace(4096)
    args = [None, da.F32, 0, d, d, None, None] + ([None] if weighted else []) + \
        [None, M, sums.data_ptr(), st.data_ptr(), ws, 4096, da.stream()]
    nat.call("dbgsom_accumulate_weighted" if weighted else "dbgsom_accumulate", *args)
    _sync()
    assert (sums.cpu().numpy() == 0).all() and int(st.cpu()[0]) == 0


# ---- 4. dbgsom_smooth at odd d --------------------------------------------------------------------------------------
def _smooth_call(nat, S, K, a, E, hop, sigma, layout, W_old):
    M, d = S.shape
    sums = da.dev(np.concatenate([S.reshape(-1), K, a, E]))
    hop_t, wo = da.dev(hop.astype(np.float32)), da.dev(W_old)
    wn = _full((M, d), float("nan"), "float64")
    chg = _full((1,), float("nan"), "float64")
    nbytes = nat.load().dbgsom_smooth_workspace_bytes(M, d)
    ws_t, ws = da.workspace(nbytes)
    nat.call("dbgsom_smooth", sums.data_ptr(), M, d, hop_t.data_ptr(), sigma, nat.LAYOUTS[layout], wo.data_ptr(),
             wn.data_ptr(), chg.data_ptr(), ws, nbytes, da.stream())
    _sync()
    return wn.cpu().numpy(), float(chg.cpu()[0])


def _check_smooth(nat, o, M, d, nan_row):
    assert d % 2 == 1 and da.gemm_splits(M, d) == da.gemm_splits(M, d + 1)
    rng = np.random.default_rng(M * 1000 + d)
    S, K, a, E, hop, W_old = da.smooth_inputs(M, d, rng, nan_row)
    sigma = 1.3
    for layout in ("compact", "aligned"):
        Wn, chg = _smooth_call(nat, S, K, a, E, hop, sigma, layout, W_old)          # smooth_gemm_generic_kernel
        Wo = o.smooth_matmul(o.gaussian_neighborhood(hop, sigma), a, o.voronoi_centers(S, K, a, layout))
        assert np.isnan(Wo).any() == nan_row
        np.testing.assert_allclose(Wn, Wo, rtol=1e-11, atol=1e-13, equal_nan=True)
        assert np.array_equal(np.isnan(Wn), np.isnan(Wo))
        if nan_row:
            assert np.isnan(chg)
        else:
            np.testing.assert_allclose(chg, o.change_total(W_old, Wo), rtol=1e-10)
        # the same call at d + 1 with a zero column takes smooth_gemm_kernel: a column's chain is the same
        zero = np.zeros((M, 1))
        We, chg_e = _smooth_call(nat, np.hstack([S, zero]), K, a, E, hop, sigma, layout, np.hstack([W_old, zero]))
        assert np.array_equal(We[:, :d], Wn, equal_nan=True)
        if not nan_row:
            assert (We[:, d] == 0).all()
            np.testing.assert_allclose(chg_e, chg, rtol=1e-12)


@pytest.mark.parametrize("M,d", sorted(da.SMOOTH_CASES))
def test_smooth_at_odd_d_is_the_oracle_and_the_dma_kernel_bit_for_bit(nat, o, M, d):
    _check_smooth(nat, o, M, d, nan_row=False)


def test_smooth_at_odd_d_gives_a_nan_row_where_every_weight_is_zero(nat, o):
    _check_smooth(nat, o, 17, 3, nan_row=True)


# ---- 5. reductions of stats.hip -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", da.SUM_N)
def test_sum_and_weighted_sum(nat, n):
    """|got - exact| <= n u sum |terms| against the exact (rational) sums; the same bits on a second call"""
    lib = nat.load()
    rng = np.random.default_rng(n)
    v, w = rng.normal(size=n) * 3.0, rng.uniform(0.0, 3.0, n)
    v_t, w_t = da.dev(v if n else np.zeros(1)), da.dev(w if n else np.zeros(1))
    nbytes = lib.dbgsom_sum_workspace_bytes()
    ws_t, ws = da.workspace(nbytes)
    for name, args, (exact, T) in (("dbgsom_sum_f64", [v_t.data_ptr()], da.exact_sum(v)),
                                   ("dbgsom_weighted_sum_f64", [v_t.data_ptr(), w_t.data_ptr()], da.exact_sum(v, w)),
                                   ("dbgsom_weighted_sum_f64", [None, w_t.data_ptr()], da.exact_sum(w))):
        got = []
        for _ in range(2):
            out = _full((1,), float("nan"), "float64")
            nat.call(name, *args, n, out.data_ptr(), ws, nbytes, da.stream())
            _sync()
            got.append(out.cpu().numpy())
        assert np.array_equal(got[0], got[1])
        err = abs(Fraction(float(got[0][0])) - exact)
        bound = n * Fraction(U) * T
        print(f"{name} n = {n}: error / bound {float(err / bound) if bound else float(err):.3f}")
        assert err <= bound


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_density_terms_and_exp_similarity(nat, o, n):
    rng = np.random.default_rng(n)
    dist = 3.0 * rng.random(n)
    dist[0] = 0.0
    d_t = da.dev(dist)
    out = _full((n,), float("nan"), "float64")
    sigma, gamma = 1.3, 0.37
    nat.call("dbgsom_density_terms", d_t.data_ptr(), n, sigma, out.data_ptr(), da.stream())
    kw = _full((n,), float("nan"), "float64")
    nat.call("dbgsom_exp_similarity", d_t.data_ptr(), n, gamma, kw.data_ptr(), da.stream())
    _sync()
    want = np.exp(-(dist ** 2) / (2 * sigma ** 2)) / (sigma * np.sqrt(2 * np.pi))
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-13)
    np.testing.assert_allclose(kw.cpu().numpy(), o.exp_similarity_gamma(dist, gamma), rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize("n", [0, 1, 5000])
@pytest.mark.parametrize("C", [1, 7])
def test_topographic_count_and_class_histogram(nat, n, C):
    rows, cols = 5, 6
    M = rows * cols
    rng = np.random.default_rng(n + C)
    idx2 = rng.integers(0, M, (max(n, 1), 2)).astype(np.int64)
    y = rng.integers(0, C, max(n, 1)).astype(np.int32)
    xy = np.array([(i, j) for i in range(rows) for j in range(cols)], dtype=np.int32)
    idx_t, y_t, xy_t = da.dev(idx2), da.dev(y), da.dev(xy)
    win_t = da.dev(idx2[:, 0])
    count = _full((1,), -1, "int64")
    hist = _full((M, C), -1, "int64")
    nat.call("dbgsom_topographic_count", idx_t.data_ptr(), n, xy_t.data_ptr(), M, count.data_ptr(), da.stream())
    nat.call("dbgsom_class_histogram", win_t.data_ptr(), y_t.data_ptr(), n, M, C, hist.data_ptr(), da.stream())
    _sync()
    pos = xy.astype(np.float64)
    apart = np.linalg.norm(pos[idx2[:n, 0]] - pos[idx2[:n, 1]], axis=1) > 1.5
    assert int(count.cpu()[0]) == int(apart.sum())
    want = np.zeros((M, C), dtype=np.int64)
    np.add.at(want, (idx2[:n, 0], y[:n]), 1)
    assert np.array_equal(hist.cpu().numpy(), want)


@pytest.mark.parametrize("N,d,ldx", da.COLSUM_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_column_sums_with_a_row_stride(nat, dtype, N, d, ldx):
    """bit-equal to a row-by-row loop in X's own dtype (np.sum may add pairwise at d = 1)"""
    rng = np.random.default_rng(N + d)
    X = da.stored(rng.normal(size=(N, d)) * 2.0 + 0.5, dtype)
    xt, xptr = da.stage(X, ldx, 0, dtype)
    mean = (da.column_sums_loop(X) / X.dtype.type(N)).astype(X.dtype)
    mean_t = da.dev(mean)
    for m_ptr, m in ((None, None), (mean_t.data_ptr(), mean)):
        out = da.dev(np.full(d, np.nan, dtype=X.dtype))
        nat.call("dbgsom_column_sums", xptr, da.CODE[dtype], N, d, ldx, m_ptr, out.data_ptr(), da.stream())
        _sync()
        assert np.array_equal(out.cpu().numpy(), da.column_sums_loop(X, m))


@pytest.mark.parametrize("N,d,ldx", da.COLSUM_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_weighted_column_sums_with_a_row_stride(nat, dtype, N, d, ldx):
    """terms w_i x_ij: one rounded product and N - 1 additions; with a mean w_i (x_ij - m_j)^2: the difference is
    exact here (float32-representable samples and means), a square, a product, N - 1 additions -- N + 1 roundings.
    Both inside (N + 2) u sum |terms| of the exact sums."""
    rng = np.random.default_rng(N + d + 1)
    vals = (rng.normal(size=(N, d)) * 2.0 + 0.5).astype(np.float32)
    X = da.stored(vals, dtype)
    Xw = np.asarray(da.widen(X), dtype=np.float64)
    w = rng.integers(0, 4, N).astype(np.float64) * rng.uniform(0.1, 2.5, N)
    mean = Xw.mean(axis=0).astype(np.float32).astype(np.float64)
    xt, xptr = da.stage(X, ldx, 0, dtype)
    w_t, mean_t = da.dev(w), da.dev(mean)
    nbytes = nat.load().dbgsom_weighted_column_sums_workspace_bytes(d)
    ws_t, ws = da.workspace(nbytes)
    L = np.longdouble
    for m_ptr, m in ((None, None), (mean_t.data_ptr(), mean)):
        out = _full((d,), float("nan"), "float64")
        nat.call("dbgsom_weighted_column_sums", xptr, da.CODE[dtype], N, d, ldx, w_t.data_ptr(), m_ptr, out.data_ptr(),
                 ws, nbytes, da.stream())
        _sync()
        base = Xw.astype(L) if m is None else (Xw.astype(L) - m.astype(L)) ** 2      # (exact: <= 50 bits)
        terms = w.astype(L)[:, None] * base
        ref, T = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        err = np.abs(out.cpu().numpy().astype(L) - ref)
        bound = (N + 2) * U * T + 2 * N * da.UL * T                                   # (+ the reference's own error)
        print(f"largest error / bound {float(np.max(err / np.where(bound > 0, bound, 1))):.3f}")
        assert np.all(err <= bound)
