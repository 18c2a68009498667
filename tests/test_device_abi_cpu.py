"""CPU: the helpers of the device-level ABI tests (tests/device_abi.py) do what they say, every shape table holds
the launcher branches it claims, the NumPy oracle alone stays inside every bound tests/test_gpu_device_abi.py
applies (its largest error / bound ratios are printed), and the argument errors of the device-level calls that
return before any HIP call come back as status codes with a message."""
import os

import numpy as np
import pytest

from tests import device_abi as da


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


@pytest.fixture(scope="module")
def lib():
    from dbgsom_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.load()


# ---- the helpers ----------------------------------------------------------------------------------------------------
def test_longdouble_has_a_64_bit_significand():
    assert da.have_longdouble()


def test_winners_with_counts_yields_the_counts_asked_for():
    rng = np.random.default_rng(0)
    for counts in (da.SEGSUM_COUNTS, da.list_counts(rng), da.group_counts(rng, 257), [0, 0, 3], [5]):
        win = da.winners_with_counts(counts, rng)
        assert win.dtype == np.int64 and np.array_equal(np.bincount(win, minlength=len(counts)), counts)
    win = da.winners_with_counts(da.SEGSUM_COUNTS, rng)
    assert not np.array_equal(win, np.sort(win))                       # shuffled: list order is not sample order


def test_staging_image_poisons_the_padding():
    rng = np.random.default_rng(1)
    for dtype in ("f32", "f64", "bf16"):
        A = da.stored(rng.normal(size=(5, 3)), dtype)
        buf = da.host_rows(A, 7, 2)
        assert buf.size == 2 + 5 * 7 and buf.dtype == A.dtype
        body = buf[2:].reshape(5, 7)
        assert np.array_equal(body[:, :3], A)
        wide = np.asarray(da.widen(buf), dtype=np.float64)
        assert np.isnan(wide[:2]).all() and np.isnan(wide[2:].reshape(5, 7)[:, 3:]).all()
        assert not np.isnan(np.asarray(da.widen(A), dtype=np.float64)).any()
    # bfloat16 bits: round to nearest even, widened exactly
    x = np.array([1.0, 1.00390625, 1.01171875, -2.5], dtype=np.float32)        # 1 + 2^-8, 1 + 3 2^-8: ties, to even
    assert da.widen(da.bf16_bits(x)).tolist() == [1.0, 1.0, 1.015625, -2.5]
    import torch

    v = rng.normal(size=1000).astype(np.float32)
    assert np.array_equal(da.widen(da.bf16_bits(v)), torch.from_numpy(v).to(torch.bfloat16).float().numpy())


def test_exact_sum_is_exact():
    import math
    from fractions import Fraction

    rng = np.random.default_rng(2)
    v, w = rng.normal(size=500) * 1e8, rng.random(500) * 1e-9
    s, t = da.exact_sum(v)
    assert float(s) == math.fsum(v) and float(t) == math.fsum(np.abs(v))
    s, t = da.exact_sum(v, w)
    assert s == sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(v, w)), Fraction(0)) and t >= abs(s)
    assert da.exact_sum(np.zeros(0)) == (0, 0)


# ---- the shape tables hold what they claim --------------------------------------------------------------------------
def test_norm_shapes_reach_both_kernels_and_their_tails():
    rows = [r for r, _, _ in da.NORM_SHAPES]
    assert max(rows) == 16385 and sorted(rows)[-2] <= 16384            # one past the switch to the 128-row kernel
    assert (17, 1025, 1031) in da.NORM_SHAPES                          # one past the 1024-wide tile
    assert any(ld > d for _, d, ld in da.NORM_SHAPES) and any(d % 16 and d > 32 for _, d, _ in da.NORM_SHAPES)


def test_bmu_cases_hold_every_vector_combination():
    for dtype in ("f32", "f64", "bf16"):
        mine = [c for c in da.BMU_CASES if c[0] == dtype]
        classes = {da.bmu_class(dt, d, d + pad, xo, 8 * wo, M) for dt, N, d, M, pad, xo, wo, k, r in mine}
        assert classes == {("reg", 0, 0), ("reg", 0, 1), ("reg", 1, 0), ("reg", 1, 1)}, (dtype, classes)
        assert {1, 3, 15, 17, 33} <= {c[2] for c in mine}
        assert {c[1] for c in mine} == {1, 127, 129} and {c[3] for c in mine} == {1, 2, 129, 257}
        assert {c[7] for c in mine} == {1, 2}
        layouts = {(pad > 0, xo) for _, _, _, _, pad, xo, _, _, _ in mine}
        assert {(False, 0), (True, 0), (False, 1)} <= layouts         # ldx = d, ldx > d, a one-element base offset
        assert all(M >= k for _, _, _, M, _, _, _, k, _ in mine)
        assert all(r == 0 or dt == "f32" for dt, _, _, _, _, _, _, _, r in mine)
    assert {c[8] for c in da.BMU_CASES} == {0, 1}
    # one W case at even d with the base 8 bytes off: the scalar W path at a d that would vectorise
    assert any(wo == 1 and d % 2 == 0 for _, _, d, _, _, _, wo, _, _ in da.BMU_CASES)
    assert 20 <= len(da.BMU_CASES) <= 40
    got = {(dt, da.bmu_class(dt, d, ldx, 0, 0, M)) for dt, N, d, M, ldx in da.BMU_DMA_CASES}
    assert got == {("f32", ("dma", 1)), ("f32", ("dma", 2)), ("f32", ("dma", 4)), ("f64", ("dma", 2))}
    assert all(ldx != d for _, _, d, _, ldx in da.BMU_DMA_CASES)
    assert ("f32", 300, 32, 40, 36) in da.BMU_DMA_CASES and ("f64", 300, 32, 40, 34) in da.BMU_DMA_CASES


def test_segsum_cases_hold_every_instantiation():
    want = {("f32", 1, "lanes"), ("f32", 1, "wide"), ("f32", 4, "lanes"), ("f32", 4, "wide"),
            ("f64", 1, "lanes"), ("f64", 1, "wide"), ("f64", 2, "lanes"), ("f64", 2, "wide"),
            ("bf16", 1, "lanes"), ("bf16", 1, "wide"), ("bf16", 8, "lanes"), ("bf16", 8, "wide")}
    got = {(dt,) + da.segsum_class(dt, d, d + pad, off) for dt, d, pad, off, _ in da.SEGSUM_CASES}
    assert got == want
    claimed = {("f32", 1, 0, 0): (1, "lanes"), ("f32", 3, 0, 0): (1, "lanes"), ("f32", 37, 0, 0): (1, "lanes"),
               ("f32", 255, 0, 0): (1, "lanes"), ("f32", 257, 0, 0): (1, "wide"), ("f32", 48, 4, 0): (4, "lanes"),
               ("f32", 1028, 0, 0): (4, "wide"), ("f32", 48, 0, 1): (1, "lanes"), ("f64", 37, 0, 0): (1, "lanes"),
               ("f64", 257, 0, 0): (1, "wide"), ("f64", 34, 2, 0): (2, "lanes"), ("f64", 514, 0, 0): (2, "wide"),
               ("bf16", 37, 0, 0): (1, "lanes"), ("bf16", 260, 1, 0): (1, "wide"), ("bf16", 64, 8, 0): (8, "lanes"),
               ("bf16", 2056, 0, 0): (8, "wide")}
    assert {c[:4] for c in da.SEGSUM_CASES} == set(claimed)
    for (dt, d, pad, off), cls in claimed.items():
        assert da.segsum_class(dt, d, d + pad, off) == cls
    # row lanes with AT % Q != 0: threads behind the last whole lane stay idle
    assert all(da.AT % d for d in (3, 37, 255))
    # weighted and unweighted for a scalar and a vector shape of every dtype
    for dt in ("f32", "f64", "bf16"):
        for weighted in (False, True):
            vs = {da.segsum_class(dt, d, d + pad, off)[0] for t, d, pad, off, w in da.SEGSUM_CASES if t == dt and w == weighted}
            assert 1 in vs and len(vs) >= 2
    # the column loop of finalize_kernel: more than 8 x 256 columns per neuron
    assert max(d for _, d, _, _, _ in da.SEGSUM_CASES) + 2 > 8 * da.AT
    counts = np.array(da.SEGSUM_COUNTS)
    assert 0 in counts and 1 in counts and da.CH in counts and (counts > 2 * da.CH).any()


def test_list_and_group_cases_hold_their_counts_and_groups():
    rng = np.random.default_rng(40)
    counts = da.list_counts(rng)
    assert counts.size == 40 and set(da.LIST_COUNTS_HEAD) <= set(counts.tolist())
    assert {0, 1, 127, 128, 129, 255, 256, 257, 128 * 33 + 1} == set(da.LIST_COUNTS_HEAD)
    assert (128 * 33 + 1 + da.CH - 1) // da.CH > da.finalize_groups(40) > 1     # more chunks than groups
    assert {M: da.finalize_groups(M) for M in da.GROUP_CASES} == da.GROUP_CASES
    assert {1, 16, 17, 256, 257, 513} == set(da.GROUP_CASES)
    for M, NG in da.GROUP_CASES.items():
        c = da.group_counts(np.random.default_rng(M), M)
        chunks = (int(c.max()) + da.CH - 1) // da.CH
        assert c.size == M and chunks >= 8
        if NG > 1:                                                     # the long list spans group boundaries
            per = (chunks + NG - 1) // NG
            assert per < chunks
    assert da.finalize_groups(256) == 2 and da.finalize_groups(257) == 1
    assert [da.hs_for(N) for N in da.SCATTER_N] == [2048, 512, 512, 512]
    case = da.histogram_case()
    n = np.bincount(case[4], minlength=case[7])
    assert case[7] == da.MAX_PROTOTYPES == 16000 and n[-1] > 0 and (n == 0).sum() > 8000 and n.sum() == 20000


def test_smooth_cases_hold_their_splits():
    assert {k: da.gemm_splits(*k) for k in da.SMOOTH_CASES} == da.SMOOTH_CASES
    assert set(da.SMOOTH_CASES.values()) >= {1, 2, 8}
    for (M, d) in da.SMOOTH_CASES:
        assert d % 2 == 1 and da.gemm_splits(M, d + 1) == da.gemm_splits(M, d)   # d only through ceil(d / 64)
        S, K, a, E, hop, W_old = da.smooth_inputs(M, d, np.random.default_rng(M * 1000 + d))
        assert hop.dtype == np.float32 and (M == 1 or np.isinf(hop).any())
        assert M == 1 or ((a == 0).any() and (S[a == 0] == 0).all() and (K[a == 0] == 0).all())


# ---- the oracle alone stays inside the bounds -----------------------------------------------------------------------
def _oracle_accumulate(o, case):
    dtype, X, ldx, off, winners, kw, dist, M, sw, integer_weights = case
    inside = (winners >= 0) & (winners < M)
    Xw, win, kw, dist = np.asarray(da.widen(X))[inside], winners[inside], kw[inside], dist[inside]
    n = np.bincount(win, minlength=M)
    if sw is None:
        S, K, a, E = o.accumulate(Xw, win, kw, dist, M)
    else:                                  # a row of weight w: the rounded factors w kw and w dist, as the kernel forms them
        w = sw[inside]
        S, K, _, E = o.accumulate(Xw, win, w * kw, w * dist, M)
    (Sr, Kr, ar, Er), (TS, TK, TE) = da.accumulate_reference(da.widen(X), winners, case[5], case[6], M, sw)
    worst = 0.0
    for name, got, ref, T in (("S", S, Sr, TS), ("K", K, Kr, TK), ("E", E, Er, TE)):
        ok, r = da.sums_within_bound(got, ref, T, n, sw is not None)
        assert ok, name
        worst = max(worst, r)
    if sw is None:
        assert np.array_equal(ar, n) and np.array_equal(a, n)
    elif integer_weights:
        assert np.array_equal(ar, np.bincount(win, weights=sw[inside], minlength=M))
    assert (np.asarray(Sr)[n == 0] == 0).all()
    return worst


def test_oracle_sums_stay_inside_the_bounds_of_the_gpu_file(o):
    cases = [("segsum " + "-".join(map(str, c)), da.segsum_case(*c)) for c in da.SEGSUM_CASES]
    cases += [(f"lists {w}", da.list_case(w)) for w in (None, "int", "frac")]
    cases += [(f"groups M={M} weighted={w}", da.group_case(M, w)) for M in sorted(da.GROUP_CASES) for w in (False, True)]
    cases += [("histogram", da.histogram_case())] + [(f"scatter N={N}", da.scatter_case(N)) for N in da.SCATTER_N]
    cases += [(f"status weighted={w} bad={b}", da.status_case(w, b)) for w in (False, True) for b in (False, True)]
    worst = 0.0
    for name, case in cases:
        r = _oracle_accumulate(o, case)
        print(f"{name}: largest error / bound {r:.3f}")
        worst = max(worst, r)
    print(f"accumulate, all cases: largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_oracle_smoothing_stays_inside_the_tolerance_of_the_gpu_file(o):
    """o.smooth_matmul (BLAS order) against the same formula in np.longdouble: rtol 1e-11, atol 1e-13"""
    L = np.longdouble
    worst = 0.0
    for (M, d) in sorted(da.SMOOTH_CASES):
        S, K, a, E, hop, W_old = da.smooth_inputs(M, d, np.random.default_rng(M * 1000 + d))
        for layout in ("compact", "aligned"):
            C = o.voronoi_centers(S, K, a, layout)
            h = o.gaussian_neighborhood(hop, 1.3)
            W = o.smooth_matmul(h, a, C)
            g = h.astype(L) * a.astype(L)[None, :]
            ref = (g @ C.astype(L)) / g.sum(axis=1)[:, None]
            assert not np.isnan(W).any()
            r = float(np.max(np.abs(W - ref) / (1e-13 + 1e-11 * np.abs(ref))))
            print(f"smooth M={M} d={d} {layout}: largest error / tolerance {r:.2e}")
            worst = max(worst, r)
    assert worst <= 1.0
    S, K, a, E, hop, W_old = da.smooth_inputs(17, 3, np.random.default_rng(17003), nan_row=True)
    with np.errstate(invalid="ignore"):
        W = o.smooth_matmul(o.gaussian_neighborhood(hop, 1.3), a, o.voronoi_centers(S, K, a, "aligned"))
    assert np.isnan(W[7]).all() and not np.isnan(np.delete(W, 7, axis=0)).any()


def test_column_sums_loop_is_numpys_axis_0_reduction():
    rng = np.random.default_rng(3)
    for dt in (np.float32, np.float64):
        X = (rng.normal(size=(513, 37)) * 2 + 0.5).astype(dt)
        assert np.array_equal(da.column_sums_loop(X), np.sum(X, axis=0))
        m = (np.sum(X, axis=0) / dt(513)).astype(dt)
        assert np.array_equal(da.column_sums_loop(X, m), np.sum((X - m) ** 2, axis=0))


# ---- argument errors that return before any HIP call ------------------------------------------------------------------
P = 0x10000          # a fake, 256-byte aligned device address: never dereferenced on these paths


def _accumulate(lib, *, d=4, ldx=4, M=5, ws=P, ws_bytes=None, N=10):
    need = lib.dbgsom_accumulate_workspace_bytes(N, d, min(M, da.MAX_PROTOTYPES))
    return lib.dbgsom_accumulate(P, da.F32, N, d, ldx, P, P, P, M, P, None, ws, need if ws_bytes is None else ws_bytes, None)


def _smooth(lib, *, M=5, d=3, sigma=1.0, layout=0, w_new=2 * P, ws=P, ws_bytes=None):
    need = lib.dbgsom_smooth_workspace_bytes(M, d)
    return lib.dbgsom_smooth(P, M, d, P, sigma, layout, P, w_new, P, ws, need if ws_bytes is None else ws_bytes, None)


def test_argument_errors_of_the_device_level_calls(lib):
    def failed(rc, code, what):
        msg = lib.dbgsom_last_error()
        assert rc == code and what in msg, (rc, msg)

    failed(_accumulate(lib, d=4, ldx=3), -1, b"bad sample shape")
    failed(lib.dbgsom_row_sqnorms(P, da.F32, 10, 4, 3, P, None), -1, b"bad shape")
    failed(lib.dbgsom_bmu(P, da.F32, 10, 4, 3, P, P, 5, P, 1, 0, P, P, None), -1, b"bad sample shape")
    failed(lib.dbgsom_column_sums(P, da.F32, 10, 4, 3, None, P, None), -1, b"bad arguments")
    failed(_accumulate(lib, M=da.MAX_PROTOTYPES + 1), -1, b"DBGSOM_MAX_PROTOTYPES")
    failed(_accumulate(lib, ws=P + 64), -1, b"256-byte aligned")
    need = lib.dbgsom_accumulate_workspace_bytes(10, 4, 5)
    failed(_accumulate(lib, ws_bytes=need - 1), -3, b"workspace too small")
    failed(_smooth(lib, layout=9), -1, b"layout")
    failed(_smooth(lib, sigma=0.0), -1, b"sigma must be positive")
    failed(_smooth(lib, w_new=P), -1, b"alias")
    failed(_smooth(lib, ws=P + 8), -1, b"256-byte aligned")
    failed(_smooth(lib, ws_bytes=lib.dbgsom_smooth_workspace_bytes(5, 3) - 1), -3, b"workspace too small")
