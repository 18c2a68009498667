"""``metric="cosine"``: the NumPy restatement of the cosine distance of the search, a CPU stand-in backend built on it
and the shape tables the CPU and GPU tests share.  Imported by tests/test_cosine_cpu.py and tests/test_gpu_cosine.py.

The contract.  ``a_ij = <x_i, w_j>``, ``q_i = |x_i|^2`` and ``p_j = |w_j|^2`` are sequential chains ``acc = fma(x_k, w_k,
acc)``, k ascending, float32 rows widened exactly (oracle/bmu_chain.c).  Then in float64, every operation rounded on
its own: ``inv(t) = 0 if t == 0; 1 / sqrt(t) if 0 < t < inf; NaN otherwise``, ``u_i = inv(q_i)``, ``v_j = inv(p_j)``,
``c_ij = 1 - (a_ij * u_i) * v_j``, ``c > 2 -> 2``, ``not (c > 0) -> 0`` except that NaN stays NaN.

NumPy has no fma.  The chain is restated in two ways and ``dot_chain`` picks one:
  1. both operands of every product representable in float32: the product is exact in float64 (24 + 24 bits), so
     ``acc + x * w`` rounds once, as the fma does;
  2. general float64: ``fma_exact`` -- TwoProduct (Veltkamp split), TwoSum, and the sum of the two error terms rounded
     to odd before the last addition, which makes that addition round as the exact sum would.  It assumes no overflow
     and no underflow: magnitudes within 1e-3 .. 1e3 in the tests (a row that holds NaN, an infinity or 1e200 comes out
     as NaN or an infinity in q whichever way, and that is all the contract asks of it)."""
import functools

import numpy as np

from dbgsom_amd.backend import EpochResult
from oracle import som_oracle as o
from tests import device_abi as da
from tests import prototype_distances as pd
from tests.manhattan import l1_select as select          # the k smallest (value, index) per row; NaN / inf never reported

U = 2.0 ** -53
NP_DTYPE = {"f32": np.float32, "f64": np.float64}


# ---- the fma, emulated ----------------------------------------------------------------------------------------------
def _split(a):
    c = 134217729.0 * a                                   # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_exact(x, w, acc):
    """round(x * w + acc) for float64 arrays, one rounding (no overflow, no underflow)"""
    x, w, acc = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64),
                                    np.asarray(acc, dtype=np.float64))
    uh, ul = two_product(x, w)
    th, tl = two_sum(acc, uh)
    v, e = two_sum(tl, ul)
    even = (np.ascontiguousarray(v).view(np.int64) & 1) == 0
    v = np.where((e != 0.0) & even, np.nextafter(v, np.where(e > 0.0, np.inf, -np.inf)), v)   # round to odd
    return th + v


def f32_representable(A):
    A = np.asarray(A, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.all((A.astype(np.float32).astype(np.float64) == A) | ~np.isfinite(A)))


def dot_chain(X, W, exact=None):
    """(N, M) float64: acc = fma(x_k, w_k, acc), k ascending.  exact: None picks (float32-representable operands: the
    plain multiply-add; otherwise the emulation), False asserts the precondition of the plain form, True emulates."""
    X64 = np.asarray(X).astype(np.float64)
    W64 = np.asarray(W, dtype=np.float64)
    plain = f32_representable(X64) and f32_representable(W64)
    if exact is None:
        exact = not plain
    assert exact or plain, "the plain multiply-add is the fma only for float32-representable operands"
    acc = np.zeros((X64.shape[0], W64.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(X64.shape[1]):
            x, w = X64[:, k, None], W64[None, :, k]
            acc = fma_exact(x, w, acc) if exact else acc + x * w
    return acc


def sqnorm_chain(A, exact=None):
    """(rows,) float64: acc = fma(a_k, a_k, acc), k ascending"""
    A64 = np.asarray(A).astype(np.float64)
    plain = f32_representable(A64)
    if exact is None:
        exact = not plain
    assert exact or plain
    acc = np.zeros(A64.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(A64.shape[1]):
            acc = fma_exact(A64[:, k], A64[:, k], acc) if exact else acc + A64[:, k] * A64[:, k]
    return acc


# ---- oracle -----------------------------------------------------------------------------------------------------------
def inv_norms(t):
    t = np.asarray(t, dtype=np.float64)
    out = np.full(t.shape, np.nan)
    out[t == 0.0] = 0.0
    ok = (t > 0.0) & (t < np.inf)
    out[ok] = 1.0 / np.sqrt(t[ok])
    return out


def cosine_from_parts(a, q, p):
    with np.errstate(invalid="ignore", over="ignore"):
        s = (a * inv_norms(q)[:, None]) * inv_norms(p)[None, :]
        c = 1.0 - s
        c = np.where(c > 2.0, 2.0, c)
        c = np.where(~(c > 0.0) & ~np.isnan(c), 0.0, c)
    return c


def cosine_distances(X, W, exact=None):
    """(N, M) float64: the contract's c_ij"""
    return cosine_from_parts(dot_chain(X, W, exact), sqnorm_chain(X, exact), sqnorm_chain(np.asarray(W, dtype=np.float64), exact))


def cosine_bmu(X, W, k=1):
    """-> (distances, winners) in ``bmu``'s shapes: (N,) for k = 1, (N, k) otherwise"""
    dist, idx = select(cosine_distances(X, W), k)
    if k == 1:
        return dist.reshape(-1), idx.reshape(-1)
    return dist, idx


def error_bound(d):
    """|c - exact| <= (2 d + 10) u absolute: d u from the dot chain (Cauchy-Schwarz on sum |x_k w_k| against |x| |w|),
    (d / 2 + 2) u from each inverse norm, 2 u from the two products, 2 u from the subtraction"""
    return (2 * d + 10) * U


def cosine_longdouble(X, W):
    Xl, Wl = np.asarray(X).astype(np.longdouble), np.asarray(W).astype(np.longdouble)
    nx, nw = np.sqrt((Xl * Xl).sum(axis=1)), np.sqrt((Wl * Wl).sum(axis=1))
    return 1 - (Xl @ Wl.T) / nx[:, None] / nw[None, :]


# ---- CPU stand-in backend ---------------------------------------------------------------------------------------------
class CosineOracleBackend(o.OracleBackend):
    """OracleBackend with the four cosine methods in NumPy (TESTS ONLY): the epoch is the oracle's sums and smoothing on
    the cosine winners and distances.  Counts its calls."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.cosine_epochs = 0
        self.cosine_queries = 0
        self.euclidean_epochs = 0
        self.reduced_on = {}          # the prototypes the reductions over the resident rows were last taken on

    def quantization_error(self, W):
        self.reduced_on["quantization_error"] = np.array(W, dtype=np.float64)
        return super().quantization_error(W)

    def topographic_error_count(self, W, coords):
        self.reduced_on["topographic_error"] = (np.array(W, dtype=np.float64), np.array(coords, dtype=np.float64))
        return super().topographic_error_count(W, coords)

    def bmu(self, W, k=1, X=None):
        if X is None and self._metric == "cosine":
            return cosine_bmu(self._X, W, k)
        return super().bmu(W, k, X)

    def bmu_cosine(self, W, k, X):
        self.cosine_queries += 1
        return cosine_bmu(np.asarray(X), W, k)

    def distances_cosine(self, W, X):
        self.cosine_queries += 1
        return cosine_distances(np.asarray(X), W)

    def kneighbors_cosine(self, W, k, X):
        self.cosine_queries += 1
        return select(cosine_distances(np.asarray(X), W), k)

    def epoch(self, *args, **kwargs):
        assert self._metric == "euclidean", "the ordinary epoch under metric='cosine'"
        self.euclidean_epochs += 1
        return super().epoch(*args, **kwargs)

    def epoch_cosine(self, W, hop, sigma, gamma, layout="compact", want_assignments=False, n_classes=0):
        assert self._metric == "cosine"
        self.cosine_epochs += 1
        dist, win = cosine_bmu(self._X, W, 1)
        kw = o.exp_similarity_gamma(dist, gamma)
        Wn, chg, E, a = self._smooth(self._sums_from(W, kw, win, dist), W, hop, sigma, layout)
        res = EpochResult(Wn, chg, E, a, win if want_assignments else None, dist if want_assignments else None)
        if n_classes > 0:
            res.class_hist = self.class_histogram(win, n_classes, np.asarray(W).shape[0])
        return res

    def release(self):
        self._metric = "euclidean"
        super().release()


# ---- shape tables -------------------------------------------------------------------------------------------------------
# restatement against extended precision and scikit-learn: N x M pairs at these d, three kinds of data
RESTATEMENT_N, RESTATEMENT_M = 300, 70
RESTATEMENT_D = [1, 3, 16, 64, 100, 784, 2049]
RESTATEMENT_KINDS = ["f32 blobs", "non-negative", "general f64"]

# the raw device calls: the table of dbgsom_distances without its bfloat16 lines (no cosine form of those)
CASES = [c for c in pd.CASES if c[0] != "bf16"]
CASE_IDS = ["%s-N%d-M%d-d%d-pad%d-xoff%d-ldo+%d-ooff%d" % c for c in CASES]
launcher_form = pd.launcher_form


def restatement_data(kind, d):
    rng = np.random.default_rng(d + 7 * RESTATEMENT_KINDS.index(kind))
    N, M = RESTATEMENT_N, RESTATEMENT_M
    if kind == "f32 blobs":
        X = (rng.normal(size=(N, d)) + 3.0 * rng.integers(0, 4, (N, 1))).astype(np.float32)
        W = rng.normal(size=(M, d)).astype(np.float32).astype(np.float64) + 1.0
    elif kind == "non-negative":
        X = rng.uniform(1e-3, 10.0, (N, d))
        W = rng.uniform(1e-3, 10.0, (M, d))
    else:
        X = rng.normal(size=(N, d)) * 3.0
        W = rng.normal(size=(M, d)) * 0.5
    return X, W


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> (X as stored, W, C): the inputs of a table entry and the oracle's matrix, computed once and shared (read
    only).  General float64 where d <= 48 (float32 rows against float64 prototypes), float32-representable at d = 784,
    so the oracle stays cheap.  With N >= 3 row 0 is zero; with M >= 4 the last prototype duplicates the first,
    prototype 1 is twice prototype 0 (collinear), and prototype M // 2 is row N // 2 of X."""
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    rng = np.random.default_rng(1000 * N + 10 * M + d + len(dtype))
    X = rng.normal(size=(N, d)) * rng.uniform(0.5, 3.0, size=d)
    W = rng.normal(size=(M, d)) * 1.5
    if d > 48:
        X, W = X.astype(np.float32).astype(np.float64), W.astype(np.float32).astype(np.float64)
    X = da.stored(X, dtype)
    if N >= 3:
        X[0] = 0.0
    if M >= 4:
        W[M - 1] = W[0]
        W[1] = 2.0 * W[0]
        W[M // 2] = X[N // 2].astype(np.float64)
    C = cosine_distances(X, W)
    for a in (X, W, C):
        a.setflags(write=False)
    return X, W, C


# the estimator fits of both test files: rows around random directions, on which the map grows under the metric.  The
# "se" threshold is 150 * -ln(spreading_factor) * |std(X)| while a neuron's error is a sum of cosine distances below 2:
# at the default 0.5 the map never grows past its four start neurons here; at 0.9 it grows to 14.  (At 0.95 it hits
# max_neurons while still moving by more than its own size per epoch, and the stand-in's fit is then ill-conditioned in
# itself: a relative perturbation of 1e-15 of each epoch's prototypes changes the number of neurons it ends with.  At
# 0.9 the same perturbation moves the prototypes by 1e-15.)
FIT_KW = dict(random_state=0, n_iter=15, max_neurons=20, spreading_factor=0.9)
N_CLASSES = 6


@functools.lru_cache(maxsize=None)
def angular_blobs(N=600, d=16):
    """N float32 rows around N_CLASSES random directions in d features, of lengths between 0.5 and 2, and their labels
    (read only)"""
    rng = np.random.default_rng(11)
    centres = rng.normal(size=(N_CLASSES, d))
    centres /= np.linalg.norm(centres, axis=1)[:, None]
    lab = rng.integers(0, N_CLASSES, N)
    X = centres[lab] + 0.12 * rng.normal(size=(N, d))
    X *= rng.uniform(0.5, 2.0, (N, 1))
    X = X.astype(np.float32)
    X.setflags(write=False)
    lab.setflags(write=False)
    return X, lab
