"""Fit on rows with missing entries (``missing_values="nan-fit"``): the NumPy restatement of one masked epoch, a CPU
stand-in backend built on it, and the inputs the CPU and GPU tests share.  Imported by tests/test_masked_fit_cpu.py
and tests/test_gpu_masked_fit.py; built on ``masked_bmu`` of tests/test_missing_cpu.py."""
import functools
from dataclasses import dataclass

import numpy as np

from dbgsom_amd.backend import EpochResult
from oracle import som_oracle as o
from tests import device_abi as da
from tests.test_missing_cpu import MaskedOracleBackend, masked_bmu

# tolerances between device and oracle on new prototypes: those of tests/test_gpu_parity.py
W_RTOL, W_ATOL = 1e-11, 1e-13


# ---- oracle -------------------------------------------------------------------------------------------------------
def masked_sums(X, winners, kw, dist, M):
    """(S, K, A, a, E) in float64, every entry a sequential sum in row order over the rows with that winner --
    S_jc = sum kw_i x_ic, K_jc = sum kw_i, A_jc = their number over the rows that observe c; a_j, E_j = sum dist_i
    over all rows of j.  Winners outside [0, M) are skipped."""
    X64 = np.asarray(X).astype(np.float64)
    winners = np.asarray(winners, dtype=np.int64)
    ok = (winners >= 0) & (winners < M)
    X64, win = X64[ok], winners[ok]
    kw, dist = np.asarray(kw, dtype=np.float64)[ok], np.asarray(dist, dtype=np.float64)[ok]
    obs = ~np.isnan(X64)
    d = X64.shape[1]
    S, K, A = np.zeros((M, d)), np.zeros((M, d)), np.zeros((M, d))
    np.add.at(S, win, kw[:, None] * np.where(obs, X64, 0.0))     # (unbuffered: row order)
    np.add.at(K, win, kw[:, None] * obs)
    np.add.at(A, win, obs.astype(np.float64))
    a = np.bincount(win, minlength=M).astype(np.float64)
    E = np.zeros(M)
    np.add.at(E, win, dist)
    return S, K, A, a, E


def masked_sums_longdouble(X, winners, kw, dist, M):
    """The same sums in np.longdouble with the sums of their terms' magnitudes, for ``device_abi.sums_within_bound``:
    -> ((S, K, A, a, E), (TS, TK, TE)); A and a exact."""
    X64 = np.asarray(X).astype(np.float64)
    winners = np.asarray(winners, dtype=np.int64)
    ok = (winners >= 0) & (winners < M)
    X64, win = X64[ok], winners[ok]
    f = np.asarray(kw, dtype=np.longdouble)[ok]
    e = np.asarray(dist, dtype=np.longdouble)[ok]
    obs = ~np.isnan(X64)
    Xz = np.where(obs, X64, 0.0).astype(np.longdouble)
    S, TS = da.segment_sums(f[:, None] * Xz, win, M)
    K, TK = da.segment_sums(f[:, None] * obs, win, M)
    A = np.asarray(da.segment_sums(obs.astype(np.float64), win, M)[0], dtype=np.float64)
    a = np.bincount(win, minlength=M).astype(np.float64)
    E, TE = da.segment_sums(e, win, M)
    return (S, K, A, a, E), (TS, TK, TE)


def masked_smooth(S, K, A, hop, sigma, W):
    """C = S / K where A > 0; W'_jc = sum_l h_jl A_lc C_lc / sum_l h_jl A_lc; W_jc where that denominator is 0."""
    W64 = np.asarray(W, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        C = np.where(A > 0, S / K, 0.0)
    h = o.gaussian_neighborhood(hop, sigma)
    num, den = h @ (A * C), h @ A
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, W64)


@dataclass
class MaskedEpochOut:
    new_weights: np.ndarray
    change_total: float
    errors: np.ndarray
    activations: np.ndarray
    winners: np.ndarray
    distances: np.ndarray
    sums: tuple       # (S, K, A)


def masked_epoch(X, W, hop, sigma, gamma, winners=None, distances=None):
    """One epoch on rows with missing entries.  winners / distances given: the sums and the smoothing
    on those instead of the oracle's own search."""
    W64 = np.asarray(W, dtype=np.float64)
    M = W64.shape[0]
    if winners is None:
        distances, winners = masked_bmu(X, W64, 1)
    kw = o.exp_similarity_gamma(distances, gamma)
    S, K, A, a, E = masked_sums(X, winners, kw, distances, M)
    Wn = masked_smooth(S, K, A, hop, sigma, W64)
    return MaskedEpochOut(Wn, o.change_total(W64, Wn), E, a, np.asarray(winners), np.asarray(distances), (S, K, A))


# ---- CPU stand-in backend -----------------------------------------------------------------------------------------
class MaskedFitOracleBackend(MaskedOracleBackend):
    """MaskedOracleBackend with ``load(X, incomplete=True)``, the resident masked ``bmu`` and ``epoch_masked`` in
    NumPy (TESTS ONLY); counts its masked epochs."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.masked_epochs = 0
        self._incomplete = False

    def load(self, X, incomplete=False):
        self._incomplete = bool(incomplete)
        return super().load(X)

    def bmu(self, W, k=1, X=None):
        if X is None and self._incomplete:
            self.masked_calls += 1
            return masked_bmu(self._X, W, k)
        return super().bmu(W, k, X)

    def epoch(self, *args, **kwargs):
        assert not self._incomplete, "the ordinary epoch on rows with missing entries"
        return super().epoch(*args, **kwargs)

    def epoch_masked(self, W, hop, sigma, gamma, want_assignments=False, n_classes=0):
        assert self._incomplete
        self.masked_epochs += 1
        out = masked_epoch(self._X, W, hop, sigma, gamma)
        res = EpochResult(out.new_weights, out.change_total, out.errors, out.activations,
                          out.winners if want_assignments else None, out.distances if want_assignments else None)
        if n_classes > 0:
            res.class_hist = self.class_histogram(out.winners, n_classes, np.asarray(W).shape[0])
        return res

    def release(self):
        self._incomplete = False
        super().release()


# ---- inputs of the estimator tests --------------------------------------------------------------------------------
def mean_fill_rmse(X_true, Xn):
    """RMSE over the punched cells of filling every hole with its column's observed mean."""
    holes = np.isnan(Xn)
    fill = np.broadcast_to(np.nanmean(Xn.astype(np.float64), axis=0), Xn.shape)
    return float(np.sqrt(np.mean((fill[holes] - X_true.astype(np.float64)[holes]) ** 2)))


def impute_rmse(X_true, Xn, filled):
    holes = np.isnan(Xn)
    return float(np.sqrt(np.mean((filled.astype(np.float64)[holes] - X_true.astype(np.float64)[holes]) ** 2)))


# ---- inputs of the device-level tests -----------------------------------------------------------------------------
# dbgsom_accumulate_masked: (N, d, M, ldx, rows' offset from a 16-byte boundary in BYTES).  (257, 17, 5): unaligned,
# the scalar loads; (1000, 130, 300): 16-byte rows whose last piece reaches behind column d; (300, 1040, 3): at
# least 256 column groups in either dtype.
ACC_SHAPES = [(1, 1, 1, 1, 0), (257, 17, 5, 20, 8), (1000, 130, 300, 132, 0), (300, 1040, 3, 1040, 0)]
ACC_FRACS = [0.0, 0.3, 0.9]
SMOOTH_M = [1, 4, 37, 300]
SMOOTH_D = [3, 17, 130]
EPOCH_SHAPES = [(257, 17, 5), (1000, 130, 300), (513, 784, 260)]


@functools.lru_cache(maxsize=None)
def accumulate_case(N, d, M, frac, dtype_name):
    """-> dict(X (N x d, dtype, NaN = missing), winners, kw, dist, big, empty, blind): neuron `big` has more than
    128 rows (several chunks), `empty` none, and no row of neuron `blind[0]` observes column `blind[1]` (None where
    the shape has no room for them).  Computed once and shared (read only)."""
    rng = np.random.default_rng(7000 * N + 10 * d + M + int(10 * frac))
    X = (rng.normal(size=(N, d)) * 1.5).astype(np.dtype(dtype_name))
    if frac > 0:
        holes = rng.random((N, d)) < frac
        holes[np.arange(N), rng.integers(0, d, N)] = False
        X[holes] = np.nan
    win = rng.integers(0, M, N).astype(np.int64)
    big = empty = blind = None
    if M >= 3 and N > 200:
        big, empty, bl = 0, 1, 2
        win[win == empty] = bl
        win[:140] = big
        col = min(2, d - 1)
        X[win == bl, col] = np.nan
        blind = (bl, col)
    kw = 1.0 - rng.random(N)
    dist = 3.0 * rng.random(N)
    out = dict(X=X, winners=win, kw=kw, dist=dist, big=big, empty=empty, blind=blind)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def accumulate_reference(N, d, M, frac, dtype_name):
    c = accumulate_case(N, d, M, frac, dtype_name)
    return masked_sums_longdouble(c["X"], c["winners"], c["kw"], c["dist"], M)


def smooth_case(M, d, split=False):
    """Sums [S | K | A] with some A_lc = 0, a hop matrix (a chain; `split`: two chains with no path between them,
    and column 0 observed by the first only) and old prototypes -> (S, K, A, a, E, hop, W_old, sigma)."""
    rng = np.random.default_rng(100 * M + d + (7 if split else 0))
    A = rng.integers(0, 6, (M, d)).astype(np.float64)
    A[rng.random((M, d)) < 0.2] = 0.0
    pos = np.arange(M, dtype=np.float64)
    hop = np.abs(pos[:, None] - pos[None, :])
    if split:
        half = M // 2
        hop[:half, half:] = np.inf
        hop[half:, :half] = np.inf
        A[half:, 0] = 0.0
        A[0, 0] = 3.0
    K = np.where(A > 0, A * rng.uniform(0.2, 1.0, (M, d)), 0.0)
    S = K * rng.normal(size=(M, d)) * 2.0
    a = A.max(axis=1) + 1.0
    E = rng.random(M)
    W_old = rng.normal(size=(M, d))
    return S, K, A, a, E, hop, W_old, 1.3
