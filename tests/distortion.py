"""Helpers of the distortion tests (tests/test_distortion_cpu.py, tests/test_gpu_distortion.py): the NumPy restatement
of the energy kernel of csrc/distortion.hip, the exact matrix of squared values it runs on, the tables of the raw device
calls and a CPU stand-in backend.

The contract (include/dbgsom_hip.h).  Row i has the squared values r_j = max((|x|^2 + (-2 <x, w_j>)) + |w_j|^2, 0), the
search's own chain (tests/cosine.py: dot_chain / sqnorm_chain).  b is the index of the smallest (r_j, j) among r_j < +inf
(none: b = -1, e = NaN); lane l of 64 adds p_l = p_l + (H[b, j] * r_j) over j = l, l + 64, ... ascending from +0.0, the
product rounded and then the sum; six rounds m = 1 .. 32 in which every lane takes p_l + p_(l ^ m) follow; e = p_0."""
import functools

import numpy as np

from tests import cosine as cs
from tests import device_abi as da
from tests import kneighbors as kn
from tests import prototype_distances as pd

U = 2.0 ** -53
SENTINEL = pd.SENTINEL      # what both result buffers are filled with (bmu: as an int64 it is -1234)
BMU_SENTINEL = -1234


# ---- the restatement ------------------------------------------------------------------------------------------------
def energy_rows(R, H):
    """R: N x M squared values, H: M x M -> (b, e)"""
    N, M = R.shape
    G = -(-M // 64)
    e = np.full(N, np.nan)
    b = np.full(N, -1, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(N):
            ok = R[i] < np.inf
            if not ok.any():
                continue
            b[i] = int(np.argmin(np.where(ok, R[i], np.inf)))          # first minimum = lowest index
            t = np.zeros(G * 64)
            t[:M] = H[b[i]] * R[i]
            t = t.reshape(G, 64)
            p = np.zeros(64)
            for g in range(G):
                m = M - 64 * g if g == G - 1 else 64
                p[:m] = p[:m] + t[g, :m]
            for m in (1, 2, 4, 8, 16, 32):
                p = p + p[np.arange(64) ^ m]
            e[i] = p[0]
    return b, e


def error_bound(M, H, R, b, extra=8):
    """(ceil(M / 64) + extra) u sum_j H[b, j] r_j per row: ceil(M / 64) + 6 additions and one product rounding per term,
    first order, plus one for slack (extra = 8)"""
    return (-(-M // 64) + extra) * U * np.sum(np.asarray(H[b], dtype=np.longdouble) * R, axis=1)


def longdouble_energy(R, H, b):
    return np.sum(np.asarray(H[b], dtype=np.longdouble) * np.asarray(R, dtype=np.longdouble), axis=1)


def squared_matrix(X, W):
    """(N x M) float64: the exact r of the search's chain, clamped at 0 (NaN kept); bfloat16 bit patterns are widened"""
    Xw = np.asarray(da.widen(np.asarray(X)))
    W = np.ascontiguousarray(W, dtype=np.float64)
    xx, ww, a = cs.sqnorm_chain(Xw), cs.sqnorm_chain(W), cs.dot_chain(Xw, W)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (xx[:, None] + (-2.0 * a)) + ww[None, :]
        return np.where(v > 0.0, v, np.where(np.isnan(v), v, 0.0))


def gaussian_factors(M, sigma=1.5, cols=None):
    """the neighbourhood factors of a cols-wide sheet of M units (Manhattan hops), as the estimator forms them"""
    cols = cols or max(1, int(np.sqrt(M)))
    ii, jj = np.divmod(np.arange(M), cols)
    hop = (np.abs(ii[:, None] - ii[None]) + np.abs(jj[:, None] - jj[None])).astype(np.float64)
    return np.exp(-(hop ** 2 / (2 * sigma ** 2)))


# ---- the restatement against np.longdouble: shapes and scales -------------------------------------------------------
BOUND_M = [1, 2, 63, 64, 65, 127, 129, 300, 1024, 2099]
BOUND_SCALES = [1e-6, 1.0, 1e6]


# ---- dbgsom_energy_rows: crafted matrices ---------------------------------------------------------------------------
ROWS_M = [1, 2, 63, 64, 65, 129, 257, 2099]      # the ends of a lane's stride, odd M, more than one unrolled trip
ROWS_N = [1, 3, 4, 5, 300]                       # a partly filled last workgroup (four rows each)
ROWS_CASES = [(ROWS_N[(i + t) % 5], M) for i, M in enumerate(ROWS_M) for t in (0, 2)]
ROWS_IDS = ["N%d-M%d" % c for c in ROWS_CASES]
ROWS_KINDS = 5


def rows_matrix(case):
    """-> R (N x M float64, >= 0 or +inf or NaN): random rows at three scales, and special rows -- the first five, or
    with fewer rows the kinds the case's place in the table selects:
      0  equal minima at columns 0, 63 and 64 (those the row has): the lowest index wins
      1  equal minima at columns 63 and 64 only: lane 63's entry beats lane 0's second one
      2  nothing but NaN: (-1, NaN)
      3  one +inf beside finite values: it enters the sum as it is
      4  +inf and NaN scattered"""
    N, M = case
    rng = np.random.default_rng(31 * N + M)
    R = rng.random((N, M)) * 10.0 ** rng.integers(-6, 7, size=(N, 1)) + 1e-9

    def special(row, kind):
        if kind == 0:
            R[row, [j for j in (0, 63, 64) if j < M]] = R[row].min() / 2
        elif kind == 1:
            R[row, [j for j in (63, 64) if j < M] or [0]] = R[row].min() / 2
        elif kind == 2:
            R[row] = np.nan
        elif kind == 3:
            R[row, (int(np.argmin(R[row])) + 1) % M] = np.inf
        else:
            R[row, rng.random(M) < 0.3] = np.inf
            R[row, rng.random(M) < 0.3] = np.nan

    first = ROWS_CASES.index(case) if case in ROWS_CASES else 0
    for t in range(min(N, ROWS_KINDS)):
        special(t, (first + t) % ROWS_KINDS if N < ROWS_KINDS else t)
    return R


def rows_factors(case):
    """a dense random H in (0, 1]: every h > 0"""
    N, M = case
    return 1.0 - np.random.default_rng(M).random((M, M))


# ---- dbgsom_neighborhood_energy over prototype_distances.CASES ------------------------------------------------------
SLAB_CASE = kn.SLAB_CASE                 # N = 300 (M = 33, d = 784): slab_rows = 100 gives three slabs


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """-> (R, H, b, e) of a table entry, computed once and shared (read only)"""
    X, W, _ = pd.case_data(case)
    R = squared_matrix(X, W)
    H = gaussian_factors(W.shape[0])
    b, e = energy_rows(R, H)
    for a in (R, H, b, e):
        a.setflags(write=False)
    return R, H, b, e


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------
class DistortionOracleBackend(kn.KNeighborsOracleBackend):
    """KNeighborsOracleBackend with ``neighborhood_energy`` from the restatement (TESTS ONLY); records the rows and the
    factors of every call."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.energy_rows, self.energy_H = [], []

    def neighborhood_energy(self, W, H, X):
        if hasattr(X, "toarray"):
            X = X.toarray()
        X = np.ascontiguousarray(X)
        assert not np.isnan(X).any()
        self.energy_rows.append(len(X))
        self.energy_H.append(np.array(H))
        b, e = energy_rows(squared_matrix(X, W), np.asarray(H, dtype=np.float64))
        return e, b
