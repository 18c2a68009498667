"""Helpers of the exemplars tests (tests/test_exemplars_cpu.py, tests/test_gpu_exemplars.py): the oracle of the selection
down the columns of a matrix of squared values (csrc/exemplars.hip), the tables of the raw device calls and a CPU
stand-in backend.

The contract (include/dbgsom_hip.h).  Column j keeps the k smallest (r_ij, i) in lexicographic order, ascending, i the
global row number; entries whose r is not below +inf never enter; unfilled slots hold (+inf, -1).  With owners row i is
a candidate for column j only if owner[i] == j.  The selection is a fold: the state after a block of rows is the k
smallest among what it held and the block."""
import functools

import numpy as np

from tests import distortion as ds
from tests import kneighbors as kn
from tests import prototype_distances as pd

MAX_NEIGHBORS = kn.MAX_NEIGHBORS
SENTINEL = pd.SENTINEL            # what the distance buffers are filled with
IDX_SENTINEL = kn.IDX_SENTINEL    # ... and the index buffers


def segment_rows(k):
    """rows per wavefront of topk_cols_partial_kernel<K>: cols_segment(K) = max(64, 8 K) of csrc/exemplars.hip"""
    return max(64, 8 * kn.k_instance(k))


def merge_parts(N, k):
    """parts of the first of two merge stages, 1 for a single stage: cols_parts(segments x K) of csrc/exemplars.hip"""
    Q = -(-N // segment_rows(k)) * kn.k_instance(k)
    return 1 if Q <= 2048 else -(-Q // 512)


def fold_scratch_bytes(N, M, k):
    """dbgsom_topk_cols_workspace_bytes restated: the lists of every segment and, with two stages, of every part"""
    K, S, P = kn.k_instance(k), -(-N // segment_rows(k)), merge_parts(N, k)
    up = lambda n: (n + 255) // 256 * 256   # noqa: E731
    return up(M * S * K * 8) + up(M * S * K * 4) + (up(M * P * K * 8) + up(M * P * K * 4) if P > 1 else 0)


# ---- oracle ---------------------------------------------------------------------------------------------------------
def topk_cols_oracle(R, k, owner=None, row0=0, state=None):
    """R: N x M squared values -> (r, i), both M x k: per column NumPy's lexsort on (r, i) over the state's entries
    (state: (r, i) of an earlier call, or None for an empty one) and the rows row0 .. row0 + N - 1.  Entries not below
    +inf are dropped; the result is padded with (inf, -1)."""
    R = np.asarray(R, dtype=np.float64)
    N, M = R.shape
    out_r, out_i = np.full((M, k), np.inf), np.full((M, k), -1, dtype=np.int64)
    rows = row0 + np.arange(N, dtype=np.int64)
    for j in range(M):
        r, i = R[:, j], rows
        if owner is not None:
            mine = np.asarray(owner) == j
            r, i = r[mine], i[mine]
        if state is not None:
            r, i = np.concatenate([state[0][j], r]), np.concatenate([state[1][j], i])
        with np.errstate(invalid="ignore"):
            ok = r < np.inf
        r, i = r[ok], i[ok]
        first = np.lexsort((i, r))[:k]
        out_r[j, :first.size], out_i[j, :first.size] = r[first], i[first]
    return out_r, out_i


def owners_of(R):
    """the unit of every row: the first minimum among r < +inf, -1 for a row without one"""
    with np.errstate(invalid="ignore"):
        key = np.where(R < np.inf, R, np.inf)
    own = np.argmin(key, axis=1).astype(np.int64)
    own[~(key < np.inf).any(axis=1)] = -1
    return own


def exemplars_oracle(R, k, own_cell=False):
    """-> (dist, idx) of dbgsom_exemplars on the exact squared matrix R: the square root behind the selection"""
    r, i = topk_cols_oracle(R, k, owner=owners_of(R) if own_cell else None)
    return np.sqrt(r), i


# ---- dbgsom_topk_cols: crafted matrices -----------------------------------------------------------------------------
COLS_M = [1, 5, 63, 64, 65, 129, 260]
# fewer rows than k, the ends of a segment for every K (64 rows up to K = 8, 128 at 16, 256 at 32), several segments
# and workgroups
COLS_N = [1, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 5000]
COLS_K = [1, 2, 3, 8, 9, 16, 17, 32]
OWNER_KINDS = ["none", "random", "empty-cell", "one-unit"]
# columns of more than 2048 candidates are merged in two stages: the last N with one stage and the first with two at
# K = 8 (segments of 64 rows), two stages at K = 1, 16 and 32, a last part of a few candidates only
COLS_LONG = [(16384, 5, 8, "random"), (16385, 5, 8, "none"), (140000, 3, 1, "empty-cell"), (20000, 70, 32, "none"),
             (17000, 65, 9, "one-unit"), (33000, 1, 3, "random")]


def _cols_cases():
    """(N, M, k, owner kind): every (M, k); N and the owners cycle as kneighbors.TOPK_CASES cycles N and the pitch, so
    that every N and every owner kind meets every launcher instance (tests/test_exemplars_cpu.py checks that)"""
    cases = []
    for mi, M in enumerate(COLS_M):
        for ki, k in enumerate(COLS_K):
            t = mi * len(COLS_K) + ki
            cases.append((COLS_N[(3 * mi + 5 * ki + t // 8) % len(COLS_N)], M, k, OWNER_KINDS[(mi + ki + ki // 4) % 4]))
    # every N at k = 32 (256-row segments), 16 and 8, where the table above has not met it
    have = {(c[0], kn.k_instance(c[2])) for c in cases}
    for K, M in ((32, 65), (16, 129), (8, 5)):
        for N in COLS_N:
            if (N, K) not in have:
                cases.append((N, M, K, OWNER_KINDS[len(cases) % 4]))
    return cases + COLS_LONG


COLS_CASES = _cols_cases()
COLS_IDS = ["N%d-M%d-k%d-%s" % c for c in COLS_CASES]
COLS_KINDS = 6


def cols_matrix(case):
    """-> R (N x M float64, >= 0 or +inf or NaN).  Ordinary columns are random at three scales, every other row coarsely
    rounded so that equal values abound; special columns (the first ones the matrix has, kind = column % 6):
      0  one value down the whole column: the lowest rows win, also across segments
      1  equal minima in the first and the last row
      2  nothing but NaN
      3  fewer than k entries below +inf
      4  +inf and NaN scattered
      5  ordinary"""
    N, M, k, _ = case
    rng = np.random.default_rng(7 * N + 13 * M + k)
    R = rng.random((N, M)) * 10.0 ** rng.integers(-3, 4, size=(1, M))
    R[1::2] = np.round(R[1::2], 1) + 0.05
    for j in range(min(M, 2 * COLS_KINDS)):
        kind = (j + (COLS_CASES.index(case) if M < COLS_KINDS and case in COLS_CASES else 0)) % COLS_KINDS
        if kind == 0:
            R[:, j] = 2.5
        elif kind == 1:
            R[0, j] = R[N - 1, j] = R[:, j].min() / 2
        elif kind == 2:
            R[:, j] = np.nan
        elif kind == 3:
            keep = rng.permutation(N)[:k // 2]
            vals = R[keep, j].copy()
            R[:, j] = np.where(rng.random(N) < 0.5, np.inf, np.nan)
            R[keep, j] = vals
        elif kind == 4:
            R[rng.random(N) < 0.3, j] = np.inf
            R[rng.random(N) < 0.3, j] = np.nan
    return R


def cols_owner(case):
    """-> None or N int64 units: a random assignment with some -1, one with an empty cell (unit 0, or no row at all for
    M = 1), every row in one unit (the last)"""
    N, M, k, kind = case
    rng = np.random.default_rng(N + M + k)
    if kind == "none":
        return None
    if kind == "random":
        own = rng.integers(0, M, N).astype(np.int64)
        own[rng.random(N) < 0.1] = -1
        return own
    if kind == "empty-cell":
        return (rng.integers(1, M, N) if M > 1 else np.full(N, -1)).astype(np.int64)
    return np.full(N, M - 1, dtype=np.int64)


# ---- dbgsom_exemplars over prototype_distances.CASES ----------------------------------------------------------------
SLAB_CASE = ds.SLAB_CASE                 # N = 300 (M = 33, d = 784): slab_rows = 100 gives three slabs


@functools.lru_cache(maxsize=None)
def case_reference(case, k, own_cell=False):
    """-> (dist, idx) of a table entry from the oracle on distortion.squared_matrix, computed once and shared"""
    dist, idx = exemplars_oracle(ds.case_reference(case)[0], k, own_cell)
    for a in (dist, idx):
        a.setflags(write=False)
    return dist, idx


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------
class ExemplarsOracleBackend(ds.DistortionOracleBackend):
    """DistortionOracleBackend with ``exemplars`` from the oracle on distortion.squared_matrix, owners the first minimum
    per row (TESTS ONLY); records the rows, k and own_cell of every call."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.exemplar_calls = []

    def exemplars(self, W, k, X, own_cell=False):
        if hasattr(X, "toarray"):
            X = X.toarray()
        X = np.ascontiguousarray(X)
        assert not np.isnan(X).any() and len(X) > 0
        self.exemplar_calls.append((len(X), int(k), bool(own_cell)))
        return exemplars_oracle(ds.squared_matrix(X, W), int(k), own_cell)
