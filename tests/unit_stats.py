"""Helpers of the per-unit statistics tests (tests/test_unit_stats_cpu.py, tests/test_gpu_unit_stats.py): the literal
restatement of csrc/unit_sums.hip, the tables of shapes, assignments and weights, the order-sensitive lists and a CPU
stand-in backend.

The contract (include/dbgsom_hip.h).  The list L_j of unit j holds the rows i with unit[i] == j, ascending in i, without
rows of weight 0.  A row's term is z_iv, or the product w_i * z_iv rounded once; its mass term 1.0 or w_i.  L_j is cut
into blocks of BLOCK = 128 list positions:
  P[b][v]    = (((+0.0 + t_0) + t_1) + ...)            the terms of block b, in list order
  sums[j][v] = (((+0.0 + P[0][v]) + P[1][v]) + ...)    blocks ascending; mass[j] likewise
np.add.accumulate is sequential, so `chain` below is that order literally.  Rows whose unit lies outside [0, M) are
in no list.

The error bound.  A term of unit j passes through at most 127 + ceil(n_j / 128) <= n_j + 1 additions and, with weights,
one product rounding, so against the exact sum of the same terms |sums - exact| <= (n_j + 2) u sum|terms| to first
order, u = 2^-53; np.longdouble (64-bit significand where the platform has one) stands for the exact sum, its own error
(n_j 2^-64 sum|terms|) below a thousandth of the bound."""
import functools

import numpy as np

from tests import mixture as mx

U = 2.0 ** -53
BLOCK = 128
MAX_VALUES = 16
SQUARES, NORM = 0, 1

N_LIST = [0, 1, 127, 128, 129, 130, 257, 1025]
M_LIST = [1, 3, 64, 65, 300]
V_LIST = [1, 2, 5, 16]
PADS = [0, 3]                                   # ldz = V + pad, lds = V + pad
ASSIGNMENTS = ["one", "round", "random", "mixed"]
WEIGHTS = ["none", "ones", "integers", "fractions", "zeros"]


# ---- the restatement ------------------------------------------------------------------------------------------------
def chain(T):
    """T: n x c terms -> (((+0.0 + T[0]) + T[1]) + ...) per column"""
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.vstack([np.zeros((1, T.shape[1])), T]), axis=0)[-1]


def as_rows(Z):
    Z = np.asarray(Z, dtype=np.float64)
    return Z[:, None] if Z.ndim == 1 else Z


def lists(units, w, M):
    units = np.asarray(units, dtype=np.int64)
    keep = np.ones(len(units), dtype=bool) if w is None else np.asarray(w) != 0
    return [np.flatnonzero((units == j) & keep) for j in range(M)]


def terms_of(L, Z, w):
    """-> len(L) x (V + 1): the value terms and the mass term of the rows L"""
    with np.errstate(all="ignore"):
        if w is None:
            return np.hstack([Z[L], np.ones((len(L), 1))])
        return np.hstack([w[L, None] * Z[L], w[L, None]])


def fold(units, Z, w, M, block=BLOCK):
    """-> (mass (M,), sums (M, V)), literally; block=None: one flat chain per unit"""
    Z = as_rows(Z)
    V = Z.shape[1]
    out = np.zeros((M, V + 1))
    for j, L in enumerate(lists(units, w, M)):
        T = terms_of(L, Z, w)
        if block is None:
            out[j] = chain(T)
        else:
            out[j] = chain(np.array([chain(T[b:b + block]) for b in range(0, len(L), block)]).reshape(-1, V + 1))
    return out[:, V].copy(), out[:, :V].copy()


def deviations(units, Y, C, mode):
    """(Y[i, v] - C[j, v])^2, or the root of their sum over v ascending from +0.0; +0.0 for rows outside [0, M)"""
    units, Y, C = np.asarray(units, dtype=np.int64), np.asarray(Y, dtype=np.float64), np.asarray(C, dtype=np.float64)
    N, V = Y.shape
    out = np.zeros((N, V) if mode == SQUARES else N)
    with np.errstate(all="ignore"):
        for i in range(N):
            j = units[i]
            if not 0 <= j < len(C):
                continue
            sq = [(Y[i, v] - C[j, v]) * (Y[i, v] - C[j, v]) for v in range(V)]
            if mode == SQUARES:
                out[i] = sq
            else:
                s = np.float64(0.0)
                for q in sq:
                    s = s + q
                out[i] = np.sqrt(s)
    return out


def statistics(units, Y, w, M, want_std=True, want_err=True):
    """-> (mass, mean, std, err) as HotPathBackend.unit_statistics defines them, from the literal pieces"""
    Y = as_rows(Y)
    mass, sums = fold(units, Y, w, M)
    with np.errstate(all="ignore"):
        mean = sums / mass[:, None]
        std = err = None
        if want_std:
            m2, sq = fold(units, deviations(units, Y, mean, SQUARES), w, M)
            std = np.sqrt(sq / m2[:, None])
        if want_err:
            err = fold(units, deviations(units, Y, mean, NORM)[:, None], w, M)[1][:, 0]
    return mass, mean, std, err


def bits(a):
    """the bit patterns, every NaN as one"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def longdouble_bound(units, Z, w, M):
    """-> (exact sums in np.longdouble (M, V + 1), the bound (n_j + 2) u sum|terms| (M, V + 1)); finite inputs"""
    Z = as_rows(Z)
    V = Z.shape[1]
    ref, lim = np.zeros((M, V + 1), np.longdouble), np.zeros((M, V + 1), np.longdouble)
    for j, L in enumerate(lists(units, w, M)):
        if w is None:
            T = np.hstack([Z[L], np.ones((len(L), 1))]).astype(np.longdouble)
        else:
            T = np.hstack([w[L, None].astype(np.longdouble) * Z[L].astype(np.longdouble), w[L, None].astype(np.longdouble)])
        ref[j] = T.sum(axis=0)
        lim[j] = (len(L) + 2) * np.longdouble(U) * np.abs(T).sum(axis=0)
    return ref, lim


# ---- the tables -----------------------------------------------------------------------------------------------------
def assignment(kind, N, M, rng):
    if kind == "one":                 # every row in the middle unit of M = 3: two empty units
        return np.full(N, 1, dtype=np.int64)
    if kind == "round":
        return np.arange(N, dtype=np.int64) % M
    u = rng.integers(0, M, N).astype(np.int64)
    if kind == "mixed" and N:         # entries the fold must skip: -1, M and 2^40
        bad = np.array([-1, M, 2 ** 40], dtype=np.int64)
        hit = rng.random(N) < 0.3
        hit[0] = True
        u[hit] = bad[rng.integers(0, 3, int(hit.sum()))]
    return u


def weights(kind, N, Z, rng):
    """-> (w or None, Z): under "zeros" a fifth of the rows get weight 0 and NaN or an infinity in Z"""
    if kind == "none":
        return None, Z
    if kind == "ones":
        return np.ones(N), Z
    if kind == "integers":
        return rng.integers(0, 4, N).astype(np.float64), Z
    w = rng.random(N) + 0.01
    if kind == "zeros":
        Z = Z.copy()
        off = rng.random(N) < 0.2
        if N:
            off[N // 2] = True
        w[off] = 0.0
        Z[off] = np.where(rng.random((int(off.sum()), Z.shape[1])) < 0.5, np.nan, np.inf)
    return w, Z


@functools.lru_cache(maxsize=None)
def problem(N, M, V, assign, weight):
    """-> (units, Z, w, mass, sums): one entry of the table with its restatement, computed once and shared (read only).
    Z spans seven decades, so that no two orders of a longer list give the same float."""
    if assign == "one":
        M = 3
    rng = np.random.default_rng(7 * N + 131 * M + 17 * V + 1000 * ASSIGNMENTS.index(assign) + 10000 * WEIGHTS.index(weight))
    Z = rng.normal(size=(N, V)) * 10.0 ** rng.integers(-3, 4, size=(N, 1))
    units = assignment(assign, N, M, rng)
    w, Z = weights(weight, N, Z, rng)
    mass, sums = fold(units, Z, w, M)
    out = (units, Z, w, mass, sums)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def cases_for(N):
    """the 20 (M, V, pad, assignment, weights) of one N: every assignment with every kind of weights, M, V and the
    padding rotating so that each value of each list comes up for every N"""
    out = []
    for a, assign in enumerate(ASSIGNMENTS):
        for k, weight in enumerate(WEIGHTS):
            i = 5 * a + k + N
            out.append((M_LIST[i % 5], V_LIST[(i // 2) % 4], PADS[i % 2], assign, weight))
    return out


SHAPES = [(M, V, pad) for M in M_LIST for V in V_LIST for pad in PADS]     # every pairing, at N = 1025


# ---- lists whose order shows ----------------------------------------------------------------------------------------
def three_orders():
    """one list for which the ascending chain, the descending chain and np.sum give three different floats"""
    rng = np.random.default_rng(0)
    return rng.normal(size=40) * 10.0 ** rng.integers(-3, 4, 40)


def blocked_list():
    """130 rows in one unit whose flat chain differs from the blocked one: the first block sums to 2^53, where the
    two 1.0 of the second block are lost one by one but survive as the partial sum 2.0"""
    z = np.zeros(130)
    z[0] = 2.0 ** 53
    z[128] = z[129] = 1.0
    return z


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------
class UnitStatsOracleBackend(mx.MixtureOracleBackend):
    """MixtureOracleBackend that takes CSR rows by densifying them, honours ``set_sample_weight`` in its epoch sums like
    tests/test_sample_weight_cpu.py's stand-in, and records the calls of ``unit_statistics`` / ``target_statistics``;
    both are HotPathBackend's NumPy defaults (TESTS ONLY)."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.unit_calls, self.target_calls, self.epoch_weights = [], [], []

    @staticmethod
    def _dense(X):
        return X.toarray() if X is not None and hasattr(X, "toarray") else X

    def load(self, X):
        return super().load(self._dense(X))

    def bmu(self, W, k=1, X=None):
        return super().bmu(W, k, self._dense(X))

    def kneighbors(self, W, k, X):
        return super().kneighbors(W, k, self._dense(X))

    def _local_sums(self, W, gamma, want_assignments):
        from oracle import som_oracle as o

        self.epoch_weights.append(np.array(W))
        dist, win = self._fn(self._X, np.asarray(W), 1)
        sums = self._sums_from(W, o.exp_similarity_gamma(dist, gamma), win, dist)
        return sums, (win if want_assignments else None), (dist if want_assignments else None)

    def _sums_from(self, W, sample_weights, winners, distances):
        from oracle import som_oracle as o

        if self._sw is None:
            return super()._sums_from(W, sample_weights, winners, distances)
        M, keep, w = np.asarray(W).shape[0], self._sw > 0, self._sw
        S, K, _, E = o.accumulate(self._X[keep], winners[keep], (w * sample_weights)[keep], (w * distances)[keep], M)
        return self._pack(S, K, np.bincount(winners, weights=w, minlength=M), E)

    def unit_statistics(self, units, Y, w, M, want_std=False, want_err=False):
        self.unit_calls.append((len(units), int(M), bool(want_std), bool(want_err)))
        return super().unit_statistics(units, Y, w, M, want_std, want_err)

    def target_statistics(self, winners, M, want_std=False, want_err=False):
        self.target_calls.append((len(winners), int(M)))
        return super().target_statistics(winners, M, want_std, want_err)
