"""Helpers of the device-level tests of the CSR kernels (tests/test_gpu_csr_device.py, tests/test_csr_device_cpu.py):
raw calls of the CSR section of include/dbgsom_hip.h on rows longer than a workgroup, neuron lists longer than a
chunk, prototype counts around the 256-prototype blocks of the search, empty groups of rows, matrices without a
stored entry, any d >= 1 -- what the context's inputs (about 32 stored entries per row, a padded feature count)
never reach.

The matrices come from rows_csr(): exactly the row lengths asked for, signed values, explicitly stored zeros.  The
references are those of tests/device_abi.py on ``X.toarray()``: the order-pinned chains of oracle/ bit for bit,
np.longdouble sums with the derived bound for the per-neuron sums.  The shape tables live here so that the CPU file
can check, without a GPU, that every table holds the branches of csrc/csr.hip it claims (constants restated below)."""
import numpy as np
import scipy.sparse as sp

from tests import device_abi as da

# csrc/csr.hip, restated
CR = 4                                  # rows per workgroup of the search
CT = 256                                # threads per workgroup = prototypes per block of the search
CCH = 128                               # rows per chunk of the sums
DENSIFY_GRID, DENSIFY_BLOCK = 65536, 64
TRANSPOSE_TILE = 32
TRANSPOSE_COLS_PER_LAUNCH = 65535 * TRANSPOSE_TILE
NP_DTYPE = {"f32": np.float32, "f64": np.float64}


def wt_ld(M):
    """dbgsom_csr_wt_ld"""
    return 0 if M < 1 else (M + CT - 1) // CT * CT


# ---- matrices -------------------------------------------------------------------------------------------------------
def arrays(X):
    """the three arrays as they are uploaded: indptr int64, indices int32, data in its own dtype"""
    assert X.has_canonical_format
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int32)
    data = np.ascontiguousarray(X.data)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype in (np.float32, np.float64)
    assert indptr.size == X.shape[0] + 1 and indptr[0] == 0 and indptr[-1] == indices.size == data.size
    return indptr, indices, data


def rows_csr(lengths, d, dtype, rng, stored_zeros=0):
    """canonical CSR in which row i stores exactly lengths[i] distinct ascending columns of [0, d); signed values
    (normal * 1.5), `stored_zeros` of them set to 0 and kept stored.  dtype: 'f32' / 'f64'."""
    lengths = np.asarray(lengths, dtype=np.int64)
    N = lengths.size
    assert d >= 1 and (lengths >= 0).all() and (lengths <= d).all()
    # row i keeps the lengths[i] columns its random keys rank first
    first = np.argsort(rng.random((N, d)), axis=1)
    mask = np.zeros((N, d), dtype=bool)
    np.put_along_axis(mask, first, np.arange(d)[None, :] < lengths[:, None], axis=1)
    rows, cols = np.nonzero(mask)                               # row-major: columns ascend within a row
    vals = (rng.normal(size=rows.size) * 1.5).astype(NP_DTYPE[dtype])
    assert stored_zeros <= vals.size
    if stored_zeros:
        vals[rng.choice(vals.size, stored_zeros, replace=False)] = 0
    indptr = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    X = sp.csr_matrix((vals, cols.astype(np.int32), indptr), shape=(N, d))     # (keeps the explicit zeros)
    assert X.has_canonical_format and X.nnz == int(lengths.sum()) and X.dtype == NP_DTYPE[dtype]
    arrays(X)
    return X


def sparsify(D, rng, keep=0.5):
    """the dense matrix D with about `keep` of its entries stored, the others dropped"""
    rows, cols = np.nonzero(rng.random(D.shape) < keep)
    X = sp.csr_matrix((D[rows, cols], (rows, cols)), shape=D.shape)
    assert X.has_canonical_format
    return X


def prototypes(M, d, rng, round_f32=0):
    """M finite prototypes; from M = 33 on a whole-NaN row (never wins) and two duplicated rows (ties go to the
    lowest index): the convention of tests/test_gpu_csr.py"""
    W = rng.normal(size=(M, d)) * 1.5
    if round_f32:
        W = W.astype(np.float32).astype(np.float64)
    if M >= 33:
        W[7] = np.nan
        W[20] = W[3]
        W[M - 1] = W[5]
    return W


# ---- shape tables ---------------------------------------------------------------------------------------------------
# 1. dbgsom_csr_row_sqnorms: one thread per row, CT rows per workgroup
NORM_N = [1, 255, 256, 257]
NORM_D, NORM_LONG = 6000, 5000


def norm_lengths(N, rng):
    """short random rows, an empty one, one of a single entry and -- the last row, the one behind the first workgroup
    at N = 257 -- one of NORM_LONG entries; N = 1: the long row alone"""
    lengths = rng.integers(0, 40, N)
    if N >= 3:
        lengths[N // 2], lengths[N // 3] = 0, 1
    lengths[N - 1] = NORM_LONG
    return lengths


# 2. dbgsom_csr_transpose_weights: (M, d, ldw); tiles of 32 x 32, ldwt / 32 tiles across
TRANSPOSE_SHAPES = [(1, 1, 1), (31, 33, 33), (32, 32, 35), (33, 31, 31), (256, 5, 8), (257, 40, 43)]
TRANSPOSE_MULTI = (3, TRANSPOSE_COLS_PER_LAUNCH + 33)      # two launches: the second of one whole tile and one column

# 3. dbgsom_bmu_csr: (dtype, N, d, M, k, round_f32)
BMU_CSR_CASES = [
    ("f32", 1, 1, 1, 1, 0), ("f64", 3, 5, 2, 2, 0), ("f32", 4, 37, 255, 1, 1), ("f64", 5, 700, 256, 2, 0),
    ("f32", 127, 5, 257, 2, 0), ("f64", 129, 37, 513, 1, 0), ("f32", 129, 700, 513, 2, 1), ("f64", 127, 700, 257, 2, 0),
    ("f32", 5, 1, 256, 2, 0), ("f64", 4, 1, 255, 2, 0), ("f32", 3, 37, 2, 1, 0), ("f64", 1, 700, 1, 1, 0),
    ("f32", 129, 5, 256, 1, 1), ("f64", 129, 700, 2, 2, 0),
]
BMU_MIX = [0, 1, 300, 700, 700, 300, 1, 0, 300, 0, 700, 1]     # rows 8 .. 19 at d = 700: three groups of mixed lengths


def search_lengths(N, d, rng):
    """row 0 stores every column; rows 4 .. 7, one group of CR rows, are empty; at d = 700 the groups behind them
    mix the lengths 0, 1, 300 and d; the rest is short and random"""
    lengths = rng.integers(0, min(d, 12) + 1, N)
    lengths[0] = d
    if N >= 2 * CR:
        lengths[CR:2 * CR] = 0
    if d == 700 and N >= 2 * CR + len(BMU_MIX):
        lengths[2 * CR:2 * CR + len(BMU_MIX)] = BMU_MIX
    return lengths


def search_case(dtype, N, d, M, k, round_f32):
    """-> (X, W)"""
    rng = np.random.default_rng(31 * N + d + M)
    lengths = search_lengths(N, d, rng)
    X = rows_csr(lengths, d, dtype, rng, stored_zeros=min(3, int(lengths.sum())))
    return X, prototypes(M, d, rng, round_f32)


TIE_BASE, TIE_M, TIE_D = 6, 516, 12       # 6 integer prototypes tiled 86 times: equal ones in three 256-blocks


def tie_case():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 5, size=(TIE_BASE, TIE_D)).astype(np.float64)
    W = np.tile(base, (TIE_M // TIE_BASE, 1))
    X = sp.csr_matrix(rng.integers(0, 5, size=(500, TIE_D)).astype(np.float64))
    assert X.has_canonical_format
    return X, W


# 4. dbgsom_csr_densify: (N, d, ld); one workgroup of 64 threads per row, 65536 workgroups at most
DENSIFY_SHAPES = [(1, 1, 1), (5, 7, 8), (9, 200, 203), (DENSIFY_GRID + 3, 5, 8)]


def densify_lengths(N, d, rng):
    if (N, d) == (9, 200):
        return np.array([200, 0, 65, 64, 1, 0, 130, 200, 0])      # a full row, second trips, empty rows
    lengths = rng.integers(0, d + 1, N)
    lengths[0] = d
    return lengths


# 5. dbgsom_accumulate_csr.  A case: (X, winners, kw, dist, M, sw, integer weights)
LONG_D, LONG_LENGTHS = 700, [0, 1, 255, 256, 257, 600, 700]


def _case(X, winners, M, rng, weights):
    _, kw, dist, sw = da.accumulate_inputs("f64", winners.size, 1, rng, weights)
    return X, winners, kw, dist, M, sw, weights != "frac"


def long_rows_case(dtype, weights):
    """d = 700, M = 6, lists of da.SEGSUM_COUNTS rows, row lengths cycling through LONG_LENGTHS"""
    rng = np.random.default_rng(700 + (dtype == "f64"))
    winners = da.winners_with_counts(da.SEGSUM_COUNTS, rng)
    lengths = np.resize(LONG_LENGTHS, winners.size)
    X = rows_csr(lengths, LONG_D, dtype, rng, stored_zeros=50)
    return _case(X, winners, len(da.SEGSUM_COUNTS), rng, weights)


LIST_SHAPES = [(20, None), (300, 280)]      # (d, stored entries per row; None: 0 .. d)


def list_case(d, per_row, weights):
    """list lengths around the chunk size: da.list_counts, M = 40"""
    rng = np.random.default_rng(40 + d)
    winners = da.winners_with_counts(da.list_counts(rng), rng)
    lengths = rng.integers(0, d + 1, winners.size) if per_row is None else np.full(winners.size, per_row)
    X = rows_csr(lengths, d, "f32", rng, stored_zeros=20)
    return _case(X, winners, 40, rng, weights)


def group_case(M, weighted):
    """second-level sum: da.group_counts, d = 8, rows of 0 .. 8 entries"""
    rng = np.random.default_rng(M)
    winners = da.winners_with_counts(da.group_counts(rng, M), rng)
    X = rows_csr(rng.integers(0, 9, winners.size), 8, "f64", rng)
    return _case(X, winners, M, rng, "int" if weighted else None)


FINALIZE_D = [2056, 1]                      # d + 2 > 8 * 256: the column loop of finalize_kernel; and the narrowest


def finalize_case(d):
    rng = np.random.default_rng(d)
    winners = da.winners_with_counts(da.SEGSUM_COUNTS, rng)
    lengths = np.resize([0, 1, 300, d] if d > 300 else [0, 1], winners.size)
    X = rows_csr(lengths, d, "f32", rng)
    return _case(X, winners, len(da.SEGSUM_COUNTS), rng, None)


def status_case(weighted, bad):
    """the data of da.status_case with about half of the entries stored"""
    _, D, d, _, winners, kw, dist, M, sw, integer = da.status_case(weighted, bad)
    return sparsify(D, np.random.default_rng(6)), winners, kw, dist, M, sw, integer


def zero_weight_nan_case():
    """long_rows_case('f64', 'int') with a NaN stored in some rows of weight 0 -> (case, rows of non-zero weight)"""
    X, winners, kw, dist, M, sw, integer = long_rows_case("f64", "int")
    lengths = np.diff(X.indptr)
    poisoned = np.flatnonzero((sw == 0) & (lengths > 0))
    assert poisoned.size >= 20
    X.data[X.indptr[poisoned]] = np.nan                          # the first stored value of each of those rows
    X.data[X.indptr[poisoned[::2] + 1] - 1] = np.nan             # and the last one of every other
    return (X, winners, kw, dist, M, sw, integer), sw != 0


# the narrowest dense rows summed column by column in list order: 256 16-byte pieces, and 256 single elements + 1
WIDE_SHAPES = [("f32", 1024), ("f64", 512), ("f32", 257), ("f64", 257)]


def wide_case(dtype, d, weighted):
    """about half of every row stored, lists of da.list_counts rows: the dense call on X.toarray() gives the same bits"""
    rng = np.random.default_rng(d)
    winners = da.winners_with_counts(da.list_counts(rng), rng)
    lengths = rng.integers(d // 2 - 40, d // 2 + 40, winners.size)
    lengths[:3] = [0, d, 1]
    X = rows_csr(lengths, d, dtype, rng, stored_zeros=100)
    return _case(X, winners, 40, rng, "int" if weighted else None)


def sums_cases():
    """(name, case, mask of the rows the reference is built from or None): every case the GPU file holds against
    da.sums_within_bound"""
    out = [(f"long rows {t} {w}", long_rows_case(t, w), None) for t in ("f32", "f64") for w in (None, "int", "frac")]
    out += [(f"lists d={d} {w}", list_case(d, per, w), None) for d, per in LIST_SHAPES for w in (None, "frac")]
    out += [(f"groups M={M} weighted={w}", group_case(M, w), None) for M in sorted(da.GROUP_CASES) for w in (False, True)]
    out += [(f"finalize d={d}", finalize_case(d), None) for d in FINALIZE_D]
    out += [(f"status weighted={w} bad={b}", status_case(w, b), None) for w in (False, True) for b in (False, True)]
    case, keep = zero_weight_nan_case()
    out.append(("weight 0 with NaN", case, keep))
    return out


# 6. through the context
CTX_N, CTX_D, CTX_M = 1500, 2048, 4


def context_lengths(rng):
    lengths = rng.integers(600, 801, CTX_N)
    lengths[[3, 500, 1499]] = 0
    lengths[[4, 777]] = CTX_D
    return lengths


# ---- the sums -------------------------------------------------------------------------------------------------------
def check_sums(case, S, K, a, E, keep=None):
    """the asserts every sums case shares: no NaN, `a` exact (integer weights) or within the bound, S / K / E inside
    da.sums_within_bound of da.accumulate_reference on X.toarray() (keep: on those rows only), empty neurons exactly
    zero.  -> largest error / bound"""
    X, winners, kw, dist, M, sw, integer_weights = case
    D = X.toarray()
    if keep is not None:
        D, winners, kw, dist, sw = D[keep], winners[keep], kw[keep], dist[keep], sw[keep]
    inside = (winners >= 0) & (winners < M)
    (Sr, Kr, ar, Er), (TS, TK, TE) = da.accumulate_reference(D, winners, kw, dist, M, sw)
    n = np.bincount(winners[inside], minlength=M)
    assert not np.isnan(S).any() and not np.isnan(K).any() and not np.isnan(a).any() and not np.isnan(E).any()
    worst = 0.0
    if sw is None:
        assert np.array_equal(a, n) and a.sum() == inside.sum()
    elif integer_weights:
        assert np.array_equal(a, np.bincount(winners[inside], weights=sw[inside], minlength=M))
    else:
        ar_, Ta = da.segment_sums(sw[inside], winners[inside], M)
        ok, worst = da.sums_within_bound(a, ar_, Ta, n, False)
        print(f"a: largest error / bound {worst:.3f}")
        assert ok
    for name, got, ref, T in (("S", S, Sr, TS), ("K", K, Kr, TK), ("E", E, Er, TE)):
        ok, r = da.sums_within_bound(got, ref, T, n, sw is not None)
        print(f"{name}: largest error / bound {r:.3f}")
        assert ok, name
        worst = max(worst, r)
    empty = n == 0
    assert (S[empty] == 0).all() and (K[empty] == 0).all() and (E[empty] == 0).all() and (a[empty] == 0).all()
    return worst


def emulate_sums(case):
    """float64 NumPy restatement of the pipeline: the stable order by winner, chunks of CCH rows added in list order
    (one rounded product and one rounded addition per term where the kernel fuses them), a neuron's chunks in chunk
    order within da.finalize_groups(M) groups, the groups in group order; rows of weight 0 are not streamed
    -> (S, K, a, E)"""
    X, winners, kw, dist, M, sw, _ = case
    D = X.toarray().astype(np.float64)
    d = D.shape[1]
    inside = (winners >= 0) & (winners < M)
    ids = np.flatnonzero(inside)
    order = ids[np.argsort(winners[ids], kind="stable")]
    counts = np.bincount(winners[ids], minlength=M)
    starts = np.r_[0, np.cumsum(counts)]
    NG = da.finalize_groups(M)
    S, K, a, E = np.zeros((M, d)), np.zeros(M), np.zeros(M), np.zeros(M)
    for j in range(M):
        rows = order[starts[j]:starts[j + 1]]
        parts = []
        for c0 in range(0, rows.size, CCH):
            acc, sk, sa, se = np.zeros(d), 0.0, 0.0, 0.0
            for r in rows[c0:c0 + CCH]:
                w = 1.0 if sw is None else sw[r]
                f, e = (kw[r], dist[r]) if sw is None else (w * kw[r], w * dist[r])
                sk, sa, se = sk + f, sa + w, se + e
                if sw is None or w != 0.0:
                    acc = acc + f * D[r]
            parts.append((acc, sk, sa, se))
        per = (len(parts) + NG - 1) // NG if parts else 0
        tot = [np.zeros(d), 0.0, 0.0, 0.0]
        for g in range(NG):
            grp = [np.zeros(d), 0.0, 0.0, 0.0]
            for p in parts[g * per:(g + 1) * per]:
                grp = [x + y for x, y in zip(grp, p)]
            tot = [x + y for x, y in zip(tot, grp)]
        S[j], K[j], a[j], E[j] = tot
    return S, K, a, E
