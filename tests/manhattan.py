"""``metric="manhattan"``: the NumPy restatement of the L1 chain, the (dist, index) selection, a CPU stand-in backend
built on them and the shape tables the CPU and GPU tests share.  Imported by tests/test_manhattan_cpu.py and
tests/test_gpu_manhattan.py.

The chain per (row, prototype) pair is ``t = x_k - w_k; acc = acc + |t|`` in float64, k ascending, float32 rows
widened exactly first.  Subtract, abs and add are correctly rounded and there is no multiply to contract, so the loop
below gives the device's bits."""
import functools

import numpy as np

from dbgsom_amd.backend import EpochResult
from oracle import som_oracle as o

U = 2.0 ** -53


# ---- oracle -------------------------------------------------------------------------------------------------------
def l1_distances(X, W):
    """(N, M) float64: sum_k |x_k - w_k|, one accumulator per pair, k ascending"""
    X64 = np.asarray(X).astype(np.float64)
    W64 = np.asarray(W, dtype=np.float64)
    acc = np.zeros((X64.shape[0], W64.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(X64.shape[1]):
            acc = acc + np.abs(X64[:, k, None] - W64[None, :, k])
    return acc


def l1_select(D, k):
    """The k smallest (dist, index) per row in lexicographic order, ascending -> (dist, idx), both (N, k).  A pair whose
    distance is not below +inf (NaN, +inf) is never reported: such slots hold (inf, -1)."""
    D = np.asarray(D, dtype=np.float64)
    N, M = D.shape
    J = np.broadcast_to(np.arange(M, dtype=np.int64), (N, M))
    key = np.where(D < np.inf, D, np.inf)             # (NaN and +inf behind every finite value)
    order = np.lexsort((J, key), axis=1)[:, :k]
    dist = np.take_along_axis(D, order, axis=1)
    idx = order.astype(np.int64)
    out = ~(dist < np.inf)
    return np.where(out, np.inf, dist), np.where(out, -1, idx)


def l1_bmu(X, W, k=1):
    """-> (distances, winners) in ``bmu``'s shapes: (N,) for k = 1, (N, k) otherwise"""
    dist, idx = l1_select(l1_distances(X, W), k)
    if k == 1:
        return dist.reshape(-1), idx.reshape(-1)
    return dist, idx


def l1_error_bound(X, W):
    """|computed - exact| <= 2 (d + 1) u * exact per pair: every term |x_k - w_k| is non-negative, one rounding in the
    subtraction and at most d in the sum (the derived bound of the issue)"""
    d = np.asarray(X).shape[1]
    return 2.0 * (d + 1) * U


# ---- CPU stand-in backend -----------------------------------------------------------------------------------------
class ManhattanOracleBackend(o.OracleBackend):
    """OracleBackend with the four Manhattan methods in NumPy (TESTS ONLY): the epoch is the oracle's sums and smoothing
    on the L1 winners and distances.  Counts its calls."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.manhattan_epochs = 0
        self.manhattan_queries = 0
        self.euclidean_epochs = 0
        self.reduced_on = {}          # the prototypes the reductions over the resident rows were last taken on

    def quantization_error(self, W):
        self.reduced_on["quantization_error"] = np.array(W, dtype=np.float64)
        return super().quantization_error(W)

    def topographic_error_count(self, W, coords):
        self.reduced_on["topographic_error"] = (np.array(W, dtype=np.float64), np.array(coords, dtype=np.float64))
        return super().topographic_error_count(W, coords)

    def bmu(self, W, k=1, X=None):
        if X is None and self._metric == "manhattan":
            return l1_bmu(self._X, W, k)
        return super().bmu(W, k, X)

    def bmu_manhattan(self, W, k, X):
        self.manhattan_queries += 1
        return l1_bmu(np.asarray(X), W, k)

    def distances_manhattan(self, W, X):
        self.manhattan_queries += 1
        return l1_distances(np.asarray(X), W)

    def kneighbors_manhattan(self, W, k, X):
        self.manhattan_queries += 1
        return l1_select(l1_distances(np.asarray(X), W), k)

    def epoch(self, *args, **kwargs):
        assert self._metric == "euclidean", "the ordinary epoch under metric='manhattan'"
        self.euclidean_epochs += 1
        return super().epoch(*args, **kwargs)

    def epoch_manhattan(self, W, hop, sigma, gamma, layout="compact", want_assignments=False, n_classes=0):
        assert self._metric == "manhattan"
        self.manhattan_epochs += 1
        dist, win = l1_bmu(self._X, W, 1)
        kw = o.exp_similarity_gamma(dist, gamma)
        Wn, chg, E, a = self._smooth(self._sums_from(W, kw, win, dist), W, hop, sigma, layout)
        res = EpochResult(Wn, chg, E, a, win if want_assignments else None, dist if want_assignments else None)
        if n_classes > 0:
            res.class_hist = self.class_histogram(win, n_classes, np.asarray(W).shape[0])
        return res

    def release(self):
        self._metric = "euclidean"
        super().release()


# ---- shape tables ---------------------------------------------------------------------------------------------------
# oracle against scikit-learn: (N, d, M), d from 1 to 2049, each in float32 and float64
SKLEARN_SHAPES = [(7, 1, 3), (33, 5, 17), (64, 33, 9), (5, 784, 12), (3, 2049, 2)]

# dbgsom_bmu_manhattan / dbgsom_distances_manhattan: (dtype, N, d, M, x pad, w pad, k).  256 prototypes per block
# (M = 255, 256, 257, 513: one block short, full, one over, three blocks); four rows per workgroup below 8192 rows
# (N = 1, 3, 4, 5, 15, 16, 17) and 16 from there on (8192 + 17 rows at d = 5, M = 3); four features per step of the
# loop (d = 1, 3, 4, 5, 7, 33).  Pairwise: every value of a dimension meets every dtype and both k.
RAW_CASES = [
    ("f32", 1, 1, 1, 0, 0, 1), ("f64", 1, 3, 2, 3, 1, 2), ("f32", 3, 4, 255, 1, 0, 2), ("f64", 3, 5, 256, 0, 3, 1),
    ("f32", 4, 7, 257, 0, 2, 1), ("f64", 4, 33, 513, 2, 0, 2), ("f32", 5, 33, 2, 3, 3, 2), ("f64", 5, 1, 255, 0, 0, 1),
    ("f32", 15, 3, 256, 0, 1, 2), ("f64", 15, 4, 257, 1, 1, 1), ("f32", 16, 5, 513, 2, 0, 1), ("f64", 16, 7, 1, 0, 2, 1),
    ("f32", 17, 7, 513, 1, 1, 2), ("f64", 17, 33, 257, 3, 0, 2), ("f64", 17, 5, 2, 0, 0, 2), ("f32", 16, 1, 256, 1, 1, 1),
    ("f32", 8192 + 17, 5, 3, 0, 0, 1), ("f64", 8192 + 17, 5, 3, 1, 1, 2),
]
NP_DTYPE = {"f32": np.float32, "f64": np.float64}


@functools.lru_cache(maxsize=None)
def raw_case(dtype, N, d, M):
    """-> (X as stored, W float64), read only.  Integers over 8 in X and over 4 in W: ties are frequent, so the order
    on equal distances is exercised at every shape, and the fractions make the sums inexact enough to need the chain."""
    rng = np.random.default_rng(1000 * N + 10 * d + M + (1 if dtype == "f32" else 0))
    X = (rng.integers(-24, 25, (N, d)) / 8.0 + rng.integers(0, 2, (N, d)) * rng.normal(size=(N, d)) * 1e-3).astype(NP_DTYPE[dtype])
    W = rng.integers(-12, 13, (M, d)) / 4.0 + rng.integers(0, 2, (M, 1)) * rng.normal(size=(M, d)) * 1e-3
    X.setflags(write=False)
    W.setflags(write=False)
    return X, W


@functools.lru_cache(maxsize=None)
def raw_reference(dtype, N, d, M):
    X, W = raw_case(dtype, N, d, M)
    D = l1_distances(X, W)
    D.setflags(write=False)
    return D


# the estimator fits of both test files: a few hundred rows of blobs on which the map grows under either metric
FIT_KW = dict(random_state=0, n_iter=15, max_neurons=20)
N_CLASSES = 6


@functools.lru_cache(maxsize=None)
def blobs():
    """400 rows of float32 blobs around 6 centres in 7 features and their labels, read only"""
    from tests import golden_inputs as gi

    X, lab = gi.blobs_f32(400, 7, 2, n_centers=N_CLASSES)
    X.setflags(write=False)
    lab.setflags(write=False)
    return X, lab
