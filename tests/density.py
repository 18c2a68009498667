"""Helpers of the density tests (tests/test_density_cpu.py, tests/test_gpu_density.py): the oracle of the count down the
columns of a matrix of squared values (csrc/density.hip), the table of crafted matrices of the raw fold, the radii of
the slab driver over the shape table of tests/prototype_distances.py, and a CPU stand-in backend.

The contract (include/dbgsom_hip.h).  counts[j, t] is the number of rows i with R[i, j] <= thr[t]: the thresholds are
squared values in any order; a NaN entry passes no threshold and a NaN threshold counts nothing; the fold ADDS to the
counts it is handed."""
import functools

import numpy as np

from dbgsom_amd.backend import squared_thresholds
from tests import distortion as ds
from tests import exemplars as ex
from tests import prototype_distances as pd

MAX_RADII = 32                       # DBGSOM_MAX_RADII
R_INSTANCES = [1, 2, 4, 8, 16, 32]   # range_count_cols_kernel<RB>: the launcher takes the smallest RB >= n_radii
LOADS = 8                            # loads in flight per lane (RANGE_LOADS)
SENTINEL = -7                        # what lies around the counts: no count is negative


def r_instance(n):
    return next(R for R in R_INSTANCES if R >= n)


def segment_rows(N, M):
    """rows per wavefront of range_count_cols_kernel: range_segment(N, G) of csrc/density.hip -- as many as leave 4096
    wavefronts on the matrix, in multiples of the unroll, between 64 and 1024"""
    G = -(-M // 64)
    return min(1024, max(64, N * G // 4096 // LOADS * LOADS))


# ---- oracle ---------------------------------------------------------------------------------------------------------
def range_counts_oracle(R, thr):
    """R: N x M squared values, thr: n thresholds -> M x n int64: a plain count_nonzero(R <= thr) per column and
    threshold"""
    R = np.asarray(R, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64).reshape(-1)
    out = np.zeros((R.shape[1], thr.size), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t, v in enumerate(thr):
            out[:, t] = np.count_nonzero(R <= v, axis=0)
    return out


# ---- dbgsom_range_count_cols: crafted matrices ----------------------------------------------------------------------
COLS_M = [1, 63, 64, 65, 257]
# one row, the ends of the unroll of eight loads, the ends of a segment of 64 rows and of a workgroup's four segments,
# several workgroups
COLS_N = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
COLS_NR = [1, 2, 3, 5, 9, 16, 31, 32]
# matrices of so many rows that a segment is longer than 64: 72 rows with a last segment of 48 and the last workgroup a
# wavefront short, 72 rows on two groups of columns, and the longest segment, 1024 rows, with a last one of 6
COLS_LONG = [(300000, 1, 2), (150000, 65, 5), (4199430, 1, 31)]


def _cols_cases():
    """(N, M, n_radii): every (M, n_radii); N cycles so that every N meets the instances 1, 8, 16 and 32 at the
    segment's ends (tests/test_density_cpu.py checks that)"""
    cases = []
    for mi, M in enumerate(COLS_M):
        for ri, n in enumerate(COLS_NR):
            cases.append((COLS_N[(3 * mi + 5 * ri + 1) % len(COLS_N)], M, n))
    have = set(cases)
    for n, M in ((32, 65), (16, 64), (5, 63), (1, 257)):          # every N at the instances 32, 16, 8 and 1
        for N in COLS_N:
            if not any(c[0] == N and r_instance(c[2]) == r_instance(n) for c in have):
                cases.append((N, M, n))
                have.add((N, M, n))
    return cases + COLS_LONG


COLS_CASES = _cols_cases()
COLS_IDS = ["N%d-M%d-n%d" % c for c in COLS_CASES]


def cols_matrix(case):
    """-> (R, thr): R N x M float64 (>= 0, +inf or NaN), thr the case's n thresholds, in no order.
    Ordinary columns are random at seven scales, every other row coarsely rounded so that equal values abound.
      thr      entries of R themselves, unsorted; with n >= 2 thr[1] duplicates thr[0], with n >= 3 thr[2] is 0.0
      planted  per threshold t, in column t % (the ordinary columns): an entry equal to it, one nextafter above and one
               nextafter below (as many of the three as the case has rows; below 0.0 there is nothing to plant)
      zeros    exact 0.0 scattered over a tenth of the entries of column 0
      M >= 3   the last column is nothing but NaN, the one before holds +inf and NaN scattered
      M == 1   every third case of the table is the NaN column"""
    N, M, n = case
    rng = np.random.default_rng(11 * N + 17 * M + n)
    R = rng.random((N, M)) * 10.0 ** rng.integers(-3, 4, size=(1, M))
    R[1::2] = np.round(R[1::2], 1) + 0.05
    thr = rng.choice(R.ravel(), n).astype(np.float64)
    if n >= 2:
        thr[1] = thr[0]
    if n >= 3:
        thr[2] = 0.0
    ordinary = max(1, M - 2)
    R[rng.random(N) < 0.1, 0] = 0.0
    for t in range(n):
        rows = rng.choice(N, min(3, N), replace=False)
        vals = [thr[t], np.nextafter(thr[t], np.inf), np.nextafter(thr[t], -np.inf)]
        for i, v in zip(rows, vals):
            if v >= 0.0:
                R[i, t % ordinary] = v
    if M >= 3:
        R[:, M - 1] = np.nan
        R[rng.random(N) < 0.3, M - 2] = np.inf
        R[rng.random(N) < 0.2, M - 2] = np.nan
    elif M == 1 and COLS_CASES.index(case) % 3 == 1:
        R[:, 0] = np.nan
    return R, thr


# ---- dbgsom_range_counts over prototype_distances.CASES -------------------------------------------------------------
SLAB_CASE = ds.SLAB_CASE                 # N = 300 (M = 33, d = 784): slab_rows = 100 gives three slabs
CASE_NR = [1, 2, 3, 5, 16, 32]


def case_nr(i):
    """the numbers of radii entry i of prototype_distances.CASES runs with: two per entry, every instance in turn"""
    return CASE_NR[i % len(CASE_NR)], CASE_NR[(i + 3) % len(CASE_NR)]


@functools.lru_cache(maxsize=None)
def case_reference(case, n):
    """-> (radii, thresholds, counts) of a table entry, computed once and shared (read only): the radii are quantiles of
    the oracle's distances (the even ones) and exact entries of them (the odd ones), unsorted; the counts are the
    oracle's on distortion.squared_matrix"""
    R = ds.case_reference(case)[0]
    D = np.sqrt(R)
    rng = np.random.default_rng(len(D.ravel()) + n)
    radii = np.quantile(D, rng.random(n))
    radii[1::2] = rng.choice(D.ravel(), n)[1::2]
    thr = squared_thresholds(radii)
    counts = range_counts_oracle(R, thr)
    for a in (radii, thr, counts):
        a.setflags(write=False)
    return radii, thr, counts


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------
class DensityOracleBackend(ex.ExemplarsOracleBackend):
    """ExemplarsOracleBackend with ``range_counts`` from the oracle on distortion.squared_matrix (TESTS ONLY); records the
    rows and the thresholds of every call."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.range_calls = []

    def range_counts(self, W, thresholds_squared, X):
        if hasattr(X, "toarray"):
            X = X.toarray()
        X = np.ascontiguousarray(X)
        assert not np.isnan(X).any() and len(X) > 0
        thr = np.array(thresholds_squared, dtype=np.float64)
        self.range_calls.append((len(X), thr))
        return range_counts_oracle(ds.squared_matrix(X, W), thr)
