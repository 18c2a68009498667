"""CPU: the helpers of the device-level CSR tests (tests/csr_device.py) do what they say, every shape table holds the
branches of csrc/csr.hip it claims (the kernels' constants restated here), a float64 NumPy restatement of the chunked,
list-order sums stays inside every bound tests/test_gpu_csr_device.py applies (its largest error / bound ratios are
printed), and the argument errors of the CSR calls that return before any HIP call come back as status codes with a
message."""
import os

import numpy as np
import pytest

from tests import csr_device as cd
from tests import device_abi as da


@pytest.fixture(scope="module")
def lib():
    from dbgsom_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.load()


# ---- rows_csr -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rows_csr_yields_the_lengths_asked_for(lib, dtype):
    rng = np.random.default_rng(0)
    lengths = np.array([0, 1, 300, 0, 299, 7, 300, 0])
    X = cd.rows_csr(lengths, 300, dtype, rng, stored_zeros=11)
    indptr, indices, data = cd.arrays(X)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == cd.NP_DTYPE[dtype]
    assert np.array_equal(np.diff(indptr), lengths) and X.shape == (8, 300) and X.has_canonical_format
    for i in range(8):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert (np.diff(cols) > 0).all() and (cols >= 0).all() and (cols < 300).all()
    assert np.array_equal(indices[indptr[2]:indptr[3]], np.arange(300))          # a full row stores every column
    assert (data == 0).sum() == 11 and X.nnz == lengths.sum()                    # stored zeros stay stored
    assert (data < 0).any() and (data > 0).any()                                 # signed
    assert lib.dbgsom_csr_check(indptr.ctypes.data, indices.ctypes.data, 8, 300, X.nnz) == 0
    assert np.array_equal(X.toarray()[2] != 0, data[indptr[2]:indptr[3]] != 0)
    # the same rows from the same generator state
    Y = cd.rows_csr(lengths, 300, dtype, np.random.default_rng(0), stored_zeros=11)
    assert np.array_equal(Y.indices, X.indices) and np.array_equal(Y.data, X.data)
    # no stored entry at all
    Z = cd.rows_csr(np.zeros(5, dtype=np.int64), 3, dtype, rng)
    zp, zi, zd = cd.arrays(Z)
    assert Z.nnz == 0 and zi.size == 0 and zd.size == 0 and (zp == 0).all()
    assert lib.dbgsom_csr_check(zp.ctypes.data, None, 5, 3, 0) == 0


def test_sparsify_and_prototypes():
    rng = np.random.default_rng(1)
    D = rng.normal(size=(50, 6))
    X = cd.sparsify(D, rng)
    T = X.toarray()
    assert 100 < X.nnz < 200 and np.array_equal(T[T != 0], D[T != 0])
    W = cd.prototypes(40, 5, rng, round_f32=1)
    assert np.isnan(W[7]).all() and np.array_equal(W[20], W[3]) and np.array_equal(W[39], W[5])
    ok = np.delete(W, 7, axis=0)
    assert np.isfinite(ok).all() and np.array_equal(ok, ok.astype(np.float32).astype(np.float64))
    assert np.isfinite(cd.prototypes(2, 5, rng)).all()


# ---- the tables hold what they claim ----------------------------------------------------------------------------------
def test_constants_of_the_kernels(lib):
    assert (cd.CR, cd.CT, cd.CCH) == (4, 256, 128) and cd.CCH == da.CH
    assert (cd.DENSIFY_GRID, cd.DENSIFY_BLOCK) == (65536, 64)
    assert cd.TRANSPOSE_COLS_PER_LAUNCH == 65535 * 32
    for M in (0, 1, 255, 256, 257, 512, 513, 16000):
        assert lib.dbgsom_csr_wt_ld(M) == cd.wt_ld(M)
    assert cd.wt_ld(0) == 0 and cd.wt_ld(1) == 256 and cd.wt_ld(256) == 256 and cd.wt_ld(257) == 512


def test_norm_and_transpose_tables():
    assert set(cd.NORM_N) == {1, cd.CT - 1, cd.CT, cd.CT + 1}
    for N in cd.NORM_N:
        lengths = cd.norm_lengths(N, np.random.default_rng(N))
        assert lengths.size == N and lengths[-1] == cd.NORM_LONG == 5000 and lengths.max() <= cd.NORM_D == 6000
        if N > 1:
            assert {0, 1} <= set(lengths.tolist())
    assert cd.TRANSPOSE_SHAPES == [(1, 1, 1), (31, 33, 33), (32, 32, 35), (33, 31, 31), (256, 5, 8), (257, 40, 43)]
    assert any(ldw > d for _, d, ldw in cd.TRANSPOSE_SHAPES) and all(ldw >= d for _, d, ldw in cd.TRANSPOSE_SHAPES)
    M, d = cd.TRANSPOSE_MULTI
    assert M == 3 and d > cd.TRANSPOSE_COLS_PER_LAUNCH
    tiles = (d + 31) // 32
    assert tiles - 65535 == 2 and d - cd.TRANSPOSE_COLS_PER_LAUNCH == 33          # a second launch: one tile + one column
    assert d * cd.wt_ld(M) * 8 < 4.4e9


def test_search_table():
    cases = cd.BMU_CSR_CASES
    assert {c[1] for c in cases} == {1, 3, 4, 5, 127, 129} and {c[3] for c in cases} == {1, 2, 255, 256, 257, 513}
    assert {c[2] for c in cases} == {1, 5, 37, 700} and {c[0] for c in cases} == {"f32", "f64"}
    assert {c[4] for c in cases} == {1, 2} and all(M >= k for _, _, _, M, k, _ in cases)
    assert all(k == 1 for _, _, _, M, k, _ in cases if M == 1)
    assert any(r for *_, r in cases) and all(t == "f32" for t, *_, r in cases if r)
    Ms = sorted({c[3] for c in cases})
    assert any(M < cd.CT for M in Ms) and cd.CT in Ms and any(cd.CT < M < 2 * cd.CT for M in Ms) and any(M > 2 * cd.CT for M in Ms)
    assert any(N % cd.CR for _, N, *_ in cases) and any(N % cd.CR == 0 for _, N, *_ in cases)
    for dt in ("f32", "f64"):                       # k = 2 across a block boundary, and at d = 700, in both types
        assert any(t == dt and M > cd.CT and k == 2 for t, _, _, M, k, _ in cases)
        assert any(t == dt and d == 700 and N >= 20 for t, N, d, *_ in cases)
    for t, N, d, M, k, r in cases:
        X, W = cd.search_case(t, N, d, M, k, r)
        lengths = np.diff(X.indptr)
        assert X.shape == (N, d) and W.shape == (M, d) and lengths[0] == d                 # a row that stores every column
        if N >= 2 * cd.CR:
            assert (lengths[cd.CR:2 * cd.CR] == 0).all()                                    # a group of four empty rows
        if d == 700 and N >= 20:
            groups = lengths[8:20].reshape(3, cd.CR)
            assert {0, 1, 300, 700} == set(groups.ravel().tolist()) and all(len(set(g.tolist())) >= 3 for g in groups)
        assert np.isnan(W).any() == (M >= 33)
        if r:
            ok = W[~np.isnan(W).any(axis=1)]
            assert np.array_equal(ok, ok.astype(np.float32).astype(np.float64))
    X, W = cd.tie_case()
    assert W.shape == (516, 12) and cd.TIE_M // cd.CT == 2 and np.array_equal(W[:6], W[510:])
    assert np.array_equal(W, np.round(W)) and np.array_equal(X.data, np.round(X.data)) and X.shape[1] == 12
    assert all(np.array_equal(W[j], W[j % 6]) for j in (6, 64 + 2, 256 + 2, 512 + 2))     # other wavefronts and blocks


def test_densify_table():
    assert cd.DENSIFY_SHAPES == [(1, 1, 1), (5, 7, 8), (9, 200, 203), (65536 + 3, 5, 8)]
    assert max(N for N, _, _ in cd.DENSIFY_SHAPES) > cd.DENSIFY_GRID
    lengths = cd.densify_lengths(9, 200, np.random.default_rng(0))
    assert lengths.max() == 200 and (lengths == 0).sum() >= 2 and {64, 65, 130} <= set(lengths.tolist())
    assert (lengths > cd.DENSIFY_BLOCK).any() and (lengths > 2 * cd.DENSIFY_BLOCK).any()
    for N, d, ld in cd.DENSIFY_SHAPES:
        assert ld >= d and cd.densify_lengths(N, d, np.random.default_rng(N + d))[0] == d


def test_sums_tables():
    for t in ("f32", "f64"):
        X, winners, kw, dist, M, sw, integer = cd.long_rows_case(t, "frac")
        lengths = np.diff(X.indptr)
        assert X.shape == (700, 700) and M == 6 and not integer and X.dtype == cd.NP_DTYPE[t]
        assert set(lengths.tolist()) == {0, 1, 255, 256, 257, 600, 700}
        assert (lengths == cd.CT).any() and (lengths > cd.CT).any() and (lengths > 2 * cd.CT).any()
        assert np.array_equal(np.bincount(winners, minlength=M), da.SEGSUM_COUNTS)
        for j in range(M):                          # every list of more than a few rows holds rows of more than 256 entries
            if da.SEGSUM_COUNTS[j] > 20:
                assert (lengths[winners == j] > cd.CT).any()
        assert (sw == 0).any() and not np.array_equal(sw, np.round(sw))
    assert cd.long_rows_case("f32", None)[5] is None and cd.long_rows_case("f32", "int")[6]
    for d, per in cd.LIST_SHAPES:
        X, winners, kw, dist, M, sw, _ = cd.list_case(d, per, None)
        counts = np.bincount(winners, minlength=M)
        assert M == 40 and set(da.LIST_COUNTS_HEAD) <= set(counts.tolist()) and X.shape[1] == d
        assert (counts < cd.CCH).any() and (counts == cd.CCH).any() and (counts > cd.CCH).any()
        assert {cd.CCH - 1, cd.CCH + 1, 2 * cd.CCH - 1, 2 * cd.CCH, 2 * cd.CCH + 1} <= set(counts.tolist())
        if per is not None:
            assert per > cd.CT and (np.diff(X.indptr) == per).all()
    assert {d for d, _ in cd.LIST_SHAPES} == {20, 300}
    for M, NG in da.GROUP_CASES.items():
        X, winners, *_ = cd.group_case(M, True)
        assert X.shape[1] == 8 and set(np.diff(X.indptr).tolist()) == set(range(9))
        assert da.finalize_groups(M) == NG and np.bincount(winners, minlength=M).max() > 7 * cd.CCH     # 8 chunks
    assert cd.FINALIZE_D == [2056, 1] and 2056 + 2 > 8 * da.AT
    assert set(np.diff(cd.finalize_case(2056)[0].indptr).tolist()) == {0, 1, 300, 2056}
    X, winners, *_ = cd.status_case(False, True)
    assert (winners == -1).sum() == 1 and (winners == 9).sum() == 1 and 0.4 < X.nnz / (1500 * 6) < 0.6
    assert cd.status_case(True, False)[1].min() >= 0 and cd.status_case(True, False)[1].max() < 9
    (X, winners, kw, dist, M, sw, _), keep = cd.zero_weight_nan_case()
    rows_with_nan = np.flatnonzero(np.isnan(X.toarray()).any(axis=1))
    assert rows_with_nan.size >= 20 and (sw[rows_with_nan] == 0).all() and not keep[rows_with_nan].any()
    assert np.array_equal(keep, sw != 0)
    assert cd.WIDE_SHAPES[:2] == [("f32", 1024), ("f64", 512)]
    assert {da.segsum_class(t, d, d, 0) for t, d in cd.WIDE_SHAPES} == {(4, "wide"), (2, "wide"), (1, "wide")}
    for t, d in cd.WIDE_SHAPES:                     # each the narrowest of its kind: one piece less goes over row lanes
        v = da.segsum_class(t, d, d, 0)[0]
        assert da.segsum_class(t, d - max(v, 2), d - max(v, 2), 0) == (v, "lanes")
    X, winners, kw, dist, M, sw, _ = cd.wide_case("f64", 512, True)
    lengths = np.diff(X.indptr)
    assert lengths[:3].tolist() == [0, 512, 1] and 0.4 < X.nnz / (X.shape[0] * 512) < 0.6 and (sw == 0).any()
    assert set(da.LIST_COUNTS_HEAD) <= set(np.bincount(winners, minlength=M).tolist())
    lengths = cd.context_lengths(np.random.default_rng(8))
    assert lengths.size == cd.CTX_N == 1500 and (lengths == 0).sum() == 3 and (lengths == cd.CTX_D).sum() == 2
    inner = lengths[(lengths > 0) & (lengths < cd.CTX_D)]
    assert inner.min() >= 600 and inner.max() <= 800 and cd.CTX_N / cd.CTX_M > 2 * cd.CCH


# ---- the restated pipeline alone stays inside the bounds ---------------------------------------------------------------
def test_emulated_chunked_sums_stay_inside_the_bounds_of_the_gpu_file():
    worst = 0.0
    for name, case, keep in cd.sums_cases():
        S, K, a, E = cd.emulate_sums(case)
        r = cd.check_sums(case, S, K, a, E, keep=keep)
        print(f"{name}: largest error / bound {r:.3f}")
        worst = max(worst, r)
    print(f"accumulate_csr, all cases: largest error / bound {worst:.3f}")
    assert 0.0 < worst <= 1.0


# ---- argument errors that return before any HIP call ------------------------------------------------------------------
P = 0x10000          # a fake, 256-byte aligned device address: never dereferenced on these paths


def test_argument_errors_of_the_csr_calls(lib):
    def failed(rc, what):
        msg = lib.dbgsom_last_error()
        assert rc == -1 and what in msg, (rc, msg)

    ld = lib.dbgsom_csr_wt_ld
    dtype = b"CSR data must be DBGSOM_F32 or DBGSOM_F64"
    failed(lib.dbgsom_csr_row_sqnorms(P, P, da.BF16, 10, P, None), dtype)
    failed(lib.dbgsom_bmu_csr(P, P, P, da.BF16, 10, P, P, ld(5), 5, P, 1, 0, P, P, None), dtype)
    failed(lib.dbgsom_csr_densify(P, P, P, da.BF16, 10, 4, 4, P, None), dtype)
    need = lib.dbgsom_accumulate_csr_workspace_bytes(10, 4, 5)
    failed(lib.dbgsom_accumulate_csr(P, P, P, da.BF16, 10, 4, P, P, None, P, 5, P, None, P, need, None), dtype)
    failed(lib.dbgsom_bmu_csr(P, P, P, da.F32, 10, P, P, ld(5), 5, P, 3, 0, P, P, None), b"k must be 1 or 2")
    failed(lib.dbgsom_bmu_csr(P, P, P, da.F32, 10, P, P, ld(1), 1, P, 2, 0, P, P, None), b"need k <= M")
    failed(lib.dbgsom_bmu_csr(P, P, P, da.F64, 10, P, P, 300, 300, P, 1, 0, P, P, None), b"ldwt must be dbgsom_csr_wt_ld(M)")
    failed(lib.dbgsom_bmu_csr(P, P, P, da.F64, 10, P, P, 1024, 300, P, 1, 0, P, P, None), b"ldwt must be dbgsom_csr_wt_ld(M)")
    failed(lib.dbgsom_csr_transpose_weights(P, 300, 4, 4, 2 * P, 1024, None), b"ldwt must be dbgsom_csr_wt_ld(M)")
    failed(lib.dbgsom_csr_transpose_weights(P, 300, 4, 4, 2 * P, 256, None), b"bad shape")          # (ldwt < M)
    failed(lib.dbgsom_csr_transpose_weights(P, 5, 4, 3, 2 * P, ld(5), None), b"bad shape")          # ldw < d
    failed(lib.dbgsom_csr_densify(P, P, P, da.F32, 10, 4, 3, P, None), b"bad shape")                # ld < d
    assert ld(0) == 0 and ld(-3) == 0
    for N, d, M in ((10, 4, 5), (700, 700, 6), (70001, 2056, 513), (1, 1, 1)):
        assert lib.dbgsom_accumulate_csr_workspace_bytes(N, d, M) == lib.dbgsom_accumulate_weighted_workspace_bytes(N, d, M) > 0
