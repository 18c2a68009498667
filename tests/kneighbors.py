"""Helpers of the kneighbors tests (tests/test_kneighbors_cpu.py, tests/test_gpu_kneighbors.py): the oracle's order
of a row's nearest prototypes, the shape tables of the raw device calls and a CPU stand-in backend.

The order comes from the oracle alone.  Distances are those of tests/prototype_distances.py (oracle/bmu_chain.c, a map
of one prototype per column); their stable arg-sort is the (r, j) order wherever two distances differ, and where they
are equal -- two different r under one square root, or a true tie -- oracle.bmu_chain on that row and the two
prototypes decides, as it decides between the two best of any search."""
import functools

import numpy as np

from oracle import som_oracle as o
from tests import device_abi as da
from tests import prototype_distances as pd
from tests.test_missing_cpu import masked_distances

MAX_NEIGHBORS = 32                     # DBGSOM_MAX_NEIGHBORS
K_INSTANCES = [1, 2, 4, 8, 16, 32]     # topk_rows_kernel<K>: the launcher takes the smallest K >= k
IDX_SENTINEL = -7                      # what the index buffers are filled with: no index is below -1


def k_instance(k):
    return next(K for K in K_INSTANCES if K >= k)


# ---- oracle -------------------------------------------------------------------------------------------------------
def _first_of_two(x_row, W, a, b):
    """whether prototype a (< b) comes before b for this row, by the oracle's own search on the two of them"""
    _, idx = o.bmu_chain(x_row[None, :], np.ascontiguousarray(W[[a, b]]), 2)
    return idx[0, 0] == 0


def topk_oracle(X, W, k, D=None):
    """-> (N x k) int64: per row the k prototypes with the smallest (r, j), ascending.  D: pair_distances(X, W) where
    the caller has it already.  Complete rows only (rows with NaN have one form of their distance, no r beside it:
    their order is the stable arg-sort of masked_distances)."""
    Xw = np.ascontiguousarray(da.widen(np.asarray(X)))
    W = np.ascontiguousarray(W, dtype=np.float64)
    if D is None:
        D = pd.pair_distances(X, W)
    M = W.shape[0]
    assert 1 <= k <= M and not np.isnan(Xw).any()
    order = np.argsort(D, axis=1, kind="stable")
    head = min(k + 1, M)
    sorted_head = np.take_along_axis(D, order[:, :head], axis=1)
    for i in np.flatnonzero((sorted_head[:, 1:] == sorted_head[:, :-1]).any(axis=1)):
        t = 0
        while t < head:
            e = t + 1
            while e < head and sorted_head[i, e] == sorted_head[i, t]:
                e += 1
            if e - t > 1:   # a run of equal distances: indices ascending (the sort is stable), re-ordered pair by pair
                run = sorted(order[i, t:e].tolist(), key=functools.cmp_to_key(
                    lambda a, b: -1 if _first_of_two(Xw[i], W, min(a, b), max(a, b)) == (a < b) else 1))
                order[i, t:e] = run
            t = e
    return np.ascontiguousarray(order[:, :k])


def masked_topk(X, W, k):
    """rows with NaN -> (dist, idx): the stable arg-sort of masked_distances"""
    D = masked_distances(X, W)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(D, idx, axis=1), idx


# ---- dbgsom_topk_rows: crafted matrices ------------------------------------------------------------------------------
TOPK_N = [1, 65, 300]
TOPK_M = [1, 5, 63, 64, 65, 260, 1000]
TOPK_K = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32]


def _topk_cases():
    """(N, M, k, ldr_pad): every (M, k) with k <= M; N and the row pitch cycle so that every (N, M), (N, k), (pad, M)
    and (pad, k) occurs too (tests/test_kneighbors_cpu.py checks that)"""
    cases = []
    for mi, M in enumerate(TOPK_M):
        for ki, k in enumerate(kk for kk in TOPK_K if kk <= M):
            cases.append((TOPK_N[(mi + ki) % 3], M, k, 3 * ((mi + ki // 3) % 2)))
    return cases


TOPK_CASES = _topk_cases()
TOPK_IDS = ["N%d-M%d-k%d-ldr+%d" % c for c in TOPK_CASES]


def topk_matrix(case):
    """-> R (N x M float64, >= 0 or +inf or NaN).  Ordinary rows are random, every other one coarsely rounded so that
    equal values abound; four kinds of special rows (the first four rows, or with N = 1 the one kind the case's place
    in the table selects): all entries equal; +inf and NaN scattered; fewer than k entries below +inf; nothing below
    +inf."""
    N, M, k, pad = case
    rng = np.random.default_rng(7 * N + 13 * M + k)
    R = rng.random((N, M)) * 10.0
    R[1::2] = np.round(R[1::2], 1)

    def special(row, kind):
        if kind == 0:
            R[row] = 2.5
        elif kind == 1:
            R[row, rng.random(M) < 0.3] = np.inf
            R[row, rng.random(M) < 0.3] = np.nan
        elif kind == 2:
            keep = rng.permutation(M)[:k // 2]
            vals = R[row, keep].copy()
            R[row] = np.where(rng.random(M) < 0.5, np.inf, np.nan)
            R[row, keep] = vals
        else:
            R[row] = np.where(rng.random(M) < 0.5, np.inf, np.nan)

    if N == 1:
        special(0, TOPK_CASES.index(case) % 4)
    else:
        for kind in range(4):
            special(kind, kind)
    return R


def topk_lexsort(R, k):
    """-> (dist, idx): NumPy's lexsort on (R, j) per row; entries not below +inf are never reported, and the slots
    they leave hold (inf, -1)"""
    N, M = R.shape
    key = np.where(R < np.inf, R, np.inf)
    idx = np.empty((N, k), dtype=np.int64)
    dist = np.empty((N, k), dtype=np.float64)
    j = np.arange(M)
    for i in range(N):
        first = np.lexsort((j, key[i]))[:k]
        ok = key[i, first] < np.inf
        idx[i] = np.where(ok, first, -1)
        dist[i] = np.where(ok, np.sqrt(key[i, first]), np.inf)
    return dist, idx


# ---- dbgsom_kneighbors over prototype_distances.CASES -----------------------------------------------------------------
KN_K = [1, 2, 5, 16, 32]


def case_ks(i):
    """the k values entry i of prototype_distances.CASES runs with (capped at its M): two per entry, so that every k
    meets both launcher forms and both store widths of the slab"""
    M = pd.CASES[i][2]
    return sorted({min(KN_K[i % 5], M), min(KN_K[(i // 5 + i + 2) % 5], M)})


SLAB_CASE = pd.CASES[5]                 # N = 300 (M = 33, d = 784) with slab_rows = 128: three slabs
COLLAPSE_X = np.array([[0.0, 0.0]])
COLLAPSE_W = np.array([[1.0, 2.0 ** -26], [1.0, 0.0], [3.0, 0.0]])   # r = 1 + 2^-52, 1, 9: sqrt(r) = 1, 1, 3


def slab_stores(case):
    """the stores of the squared kernels into the slab (always 16-byte aligned, rows M rounded up to even apart):
    '16' where M has a full group of four prototypes, '8' where M % 4 leaves a tail"""
    M = case[2]
    return ({"16"} if M >= 4 else set()) | ({"8"} if M % 4 else set())


# ---- CPU stand-in backend ----------------------------------------------------------------------------------------------
class KNeighborsOracleBackend(pd.DistancesOracleBackend):
    """DistancesOracleBackend with ``kneighbors`` / ``kneighbors_masked`` from the oracle (TESTS ONLY); records the
    rows of every call."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.kneighbors_rows, self.masked_kneighbors_rows = [], []

    def kneighbors(self, W, k, X):
        if hasattr(X, "toarray"):
            X = X.toarray()
        X = np.ascontiguousarray(X)
        assert not np.isnan(X).any()
        self.kneighbors_rows.append(len(X))
        D = pd.pair_distances(X, W)
        idx = topk_oracle(X, W, k, D)
        return np.take_along_axis(D, idx, axis=1), idx

    def kneighbors_masked(self, W, k, X):
        assert np.isnan(X).any(axis=1).all()
        self.masked_kneighbors_rows.append(len(X))
        return masked_topk(X, W, k)
