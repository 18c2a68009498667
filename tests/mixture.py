"""Helpers of the mixture tests (tests/test_mixture_cpu.py, tests/test_gpu_mixture.py): the NumPy restatement of the
rows kernel of csrc/mixture.hip, an np.longdouble evaluation of the same t_j, the error bounds, the crafted matrices of
the raw device call and a CPU stand-in backend.

The contract (include/dbgsom_hip.h).  Row i has the squared values r_j of the search's own chain
(tests/distortion.py: squared_matrix).  With log-priors a_j and c = 1 / (2 h^2):
  t_j    = a_j - (c * r_j)         the product rounded, then the difference rounded
  (T, b) = the largest t_j, lowest j among equals, over t_j > -inf and not NaN; none: (b, lse, q) = (-1, NaN, NaN)
  s_j    = exp(t_j - T)            the difference is a float64 operation, rounded
  S      = sum_j s_j               Q_v = sum_j (s_j * Y[j, v]), the product rounded, then the sum rounded
  lse    = T + log(S)              q_v = Q_v / S
Lane l of 64 adds its terms j = l, l + 64, ... ascending from +0.0; six rounds m = 1 .. 32 in which every lane takes
p_l + p_(l ^ m) follow.  A NaN t_j is never the maximum but enters the sums as it is.

The error bounds.  B(M, E) = (ceil(M / 64) + 8 + E) u, u = 2^-53, bounds the relative error of S and of Q_v (for Y >= 0;
in general relative to sum_j s_j |Y[j, v]|) against the np.longdouble evaluation on the same t_j - T: a term passes
through ceil(M / 64) - 1 + 6 additions, one product rounding and an exp of E ulp (2 E u), first order, with slack.
E_NP is the accuracy of the host's exp: glibc documents its double exp as within 1 ulp ("Errors in Math Functions" of
its manual); the manual is not installed on the machines this was written on and NumPy may take a SIMD routine of its
own (documented below 1 ulp as well), so the figure is taken as 1 from memory of both, not read off a local file.
E_DEVICE is the accuracy of the device library's float64 exp: no figure is stated in the ROCm tree, so it is twice the
largest error measured on the MI355X on these tables' own arguments.
What the kernel returns is lse and q, not S and Q_v:
  lse  |lse - ref| <= B + 2 u |ref|           log(S (1 + e)) = log S + e; log's own rounding and the addition's: 2 u |lse|
  q_v  |q_v - ref| <= (2 B + u) A_v / S       Q_v and S each within B, the division's rounding u; A_v = sum_j s_j |Y[j, v]|"""
import functools

import numpy as np

from tests import density as dn
from tests import distortion as ds
from tests import prototype_distances as pd

U = 2.0 ** -53
E_NP = 1.0
E_DEVICE = 1.75         # 2 x 0.8701, the largest measured error of the kernel's s_j in ulp, rounded up
MAX_VALUES = 16         # DBGSOM_MAX_MIXTURE_VALUES
V_INSTANCES = [0, 1, 2, 4, 8, 16]


def v_instance(n):
    return next(V for V in V_INSTANCES if V >= n)


# ---- the restatement ------------------------------------------------------------------------------------------------
def lane_sum(terms):
    """terms: M float64 -> their sum in the kernel's order"""
    M = len(terms)
    G = -(-M // 64)
    p = np.zeros(64)
    for g in range(G):
        m = M - 64 * g if g == G - 1 else 64
        p[:m] = p[:m] + terms[64 * g:64 * g + m]
    for m in (1, 2, 4, 8, 16, 32):
        p = p + p[np.arange(64) ^ m]
    return p[0]


def t_values(R, a, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(a, dtype=np.float64)[None, :] - (np.float64(c) * np.asarray(R, dtype=np.float64))


def mixture_rows(R, a, c, Y=None, parts=False):
    """R: N x M squared values, a: M log-priors, Y: M x V or None -> (b, lse, q) -- q is N x 0 for Y None --, and with
    `parts` also (S, Q, T)"""
    R = np.asarray(R, dtype=np.float64)
    N, M = R.shape
    Y = np.zeros((M, 0)) if Y is None else np.asarray(Y, dtype=np.float64)
    V = Y.shape[1]
    t = t_values(R, a, c)
    b = np.full(N, -1, np.int64)
    lse, T = np.full(N, np.nan), np.full(N, np.nan)
    q, S, Q = np.full((N, V), np.nan), np.full(N, np.nan), np.full((N, V), np.nan)
    with np.errstate(all="ignore"):
        for i in range(N):
            ok = t[i] > -np.inf                                          # (NaN: False)
            if not ok.any():
                continue
            b[i] = int(np.argmax(np.where(ok, t[i], -np.inf)))           # first maximum = lowest index
            T[i] = t[i, b[i]]
            s = np.exp(t[i] - T[i])
            S[i] = lane_sum(s)
            lse[i] = T[i] + np.log(S[i])
            for v in range(V):
                Q[i, v] = lane_sum(s * Y[:, v])
                q[i, v] = Q[i, v] / S[i]
    return (b, lse, q, S, Q, T) if parts else (b, lse, q)


def longdouble_parts(R, a, c, Y, b):
    """-> (S, Q, A, lse) in np.longdouble on the same t_j and the same rounded t_j - T, rows with b >= 0 (others NaN):
    A_v = sum_j s_j |Y[j, v]|"""
    L = np.longdouble
    t = t_values(R, a, c)
    N, M = t.shape
    Y = np.zeros((M, 0)) if Y is None else np.asarray(Y, dtype=np.float64)
    S, lse = np.full(N, np.nan, L), np.full(N, np.nan, L)
    Q, A = np.full((N, Y.shape[1]), np.nan, L), np.full((N, Y.shape[1]), np.nan, L)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(b >= 0):
            T = t[i, b[i]]
            s = np.exp((t[i] - T).astype(L))
            S[i] = s.sum()
            lse[i] = L(T) + np.log(S[i])
            Q[i] = (s[:, None] * Y.astype(L)).sum(axis=0)
            A[i] = (s[:, None] * np.abs(Y).astype(L)).sum(axis=0)
    return S, Q, A, lse


def bound(M, E):
    return (-(-M // 64) + 8 + E) * U


def defined(R, a, c):
    """the rows the model does not define as NaN: a unit with mass, and no NaN t_j"""
    t = t_values(R, a, c)
    return (t > -np.inf).any(axis=1) & ~np.isnan(t).any(axis=1)


def check_outputs(R, a, c, Y, b, lse, q, E):
    """the returned lse and q of the rows with unit b against np.longdouble, within the bounds of the docstring; every
    row the model defines takes part -> the largest error / bound seen (lse, q)"""
    M = R.shape[1]
    S, Q, A, lse_ref = longdouble_parts(R, a, c, Y, b)
    rows = defined(R, a, c)
    assert (b[rows] >= 0).all()
    B = bound(M, E)
    L = np.longdouble
    err = np.abs(lse[rows].astype(L) - lse_ref[rows])
    lim = B + 2 * U * np.abs(lse_ref[rows])
    assert (err <= lim).all(), "lse: largest error / bound = %.3f" % float(np.max(err / lim))
    worst = [float(np.max(err / lim)) if rows.any() else 0.0, 0.0]
    if q.shape[1] and rows.any():
        ref = Q[rows] / S[rows, None]
        qerr = np.abs(q[rows].astype(L) - ref)
        qlim = (2 * B + U) * A[rows] / S[rows, None]
        assert (qerr <= qlim).all(), "q: an error above its bound"
        nz = qlim > 0
        worst[1] = float(np.max(qerr[nz] / qlim[nz])) if nz.any() else 0.0
    return worst


# ---- dbgsom_mixture_rows: crafted matrices --------------------------------------------------------------------------
ROWS_M = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1025]   # both ends of a lane's stride and of the 256 values in registers
ROWS_N = [1, 4, 5, 9]                                    # four rows per workgroup
ROWS_NV = [0, 1, 2, 3, 4, 5, 8, 9, 16]                   # every instance, and counts between two instances
# (N, M, n_values, equal priors): every M with equal priors (the ties are then ties of r) and with random ones
ROWS_CASES = [(ROWS_N[(i + 3 * t) % 4], M, ROWS_NV[(2 * i + 5 * t) % 9], t == 0) for i, M in enumerate(ROWS_M) for t in (0, 1)]
ROWS_IDS = ["N%d-M%d-V%d-%s" % (c[0], c[1], c[2], "equal" if c[3] else "random") for c in ROWS_CASES]
ROWS_KINDS = 5


def rows_problem(case):
    """-> (R, a, c, Y): R N x M float64 (>= 0, +inf or NaN), random rows at seven scales under one c, so that some rows
    have every s_j but the winner's at 0 and others every s_j near 1; a the log-priors -- equal, or random with a fifth
    of them -inf (M >= 3) --; Y in (0, 1].  Special rows -- the first five, or with fewer rows the kinds the case's place
    in the table selects:
      0  equal minima of r at columns 0, 63 and 64 (those the row has): under equal priors the lowest index wins
      1  equal minima at columns 63 and 64 only: lane 63's entry beats lane 0's second one
      2  nothing but NaN: (-1, NaN, NaN)
      3  +inf in a third of the columns, never at the minimum: s = 0 there
      4  one NaN: the unit comes from the others, lse and q are NaN"""
    N, M, nv, equal = case
    rng = np.random.default_rng(1000 * N + 7 * M + nv + 31 * equal)
    R = rng.random((N, M)) * 10.0 ** rng.integers(-3, 4, size=(N, 1)) + 1e-9
    c = 2.5
    if equal:
        a = np.full(M, -np.log(M))
    else:
        w = rng.random(M) + 0.05
        if M >= 3:
            w[rng.random(M) < 0.2] = 0.0
            w[M // 2] = 0.5
        with np.errstate(divide="ignore"):
            a = np.log(w / w.sum())
    Y = 1.0 - rng.random((M, nv))

    def special(row, kind):
        if kind == 0:
            R[row, [j for j in (0, 63, 64) if j < M]] = R[row].min() / 2
        elif kind == 1:
            R[row, [j for j in (63, 64) if j < M] or [0]] = R[row].min() / 2
        elif kind == 2:
            R[row] = np.nan
        elif kind == 3:
            hit = rng.random(M) < 0.34
            hit[int(np.argmin(R[row]))] = False
            R[row, hit] = np.inf
        else:
            R[row, (int(np.argmin(R[row])) + 1) % M] = np.nan

    first = ROWS_CASES.index(case) if case in ROWS_CASES else 0
    for k in range(min(N, ROWS_KINDS)):
        special(k, (first + k) % ROWS_KINDS if N < ROWS_KINDS else k)
    return R, a, c, Y


def underflow_c(R):
    """a c so large that, under equal priors, every s_j but those of a row's minima underflows to 0: the smallest gap
    between a row's minimum and its next distinct value, times c, is above 800 > 745.2 = -log(the smallest subnormal)"""
    gaps = []
    for r in R:
        v = np.unique(r[np.isfinite(r)])
        if len(v) >= 2:
            gaps.append(v[1] - v[0])
    return 1000.0 / min(gaps) if gaps else 1.0


# ---- dbgsom_mixture over prototype_distances.CASES ------------------------------------------------------------------
SLAB_CASE = ds.SLAB_CASE                 # N = 300 (M = 33, d = 784): slab_rows = 100 gives three slabs


def case_nv(i):
    """the number of values entry i of prototype_distances.CASES runs with: every entry of ROWS_NV in turn"""
    return ROWS_NV[i % len(ROWS_NV)]


@functools.lru_cache(maxsize=None)
def case_reference(case, nv, equal=False):
    """-> (R, a, c, Y, b, lse, q) of a table entry, computed once and shared (read only): c from the mean of the row
    minima of R (h^2 = that mean / d), random priors (or equal ones), Y in (0, 1]"""
    X, W, _ = pd.case_data(case)
    R = ds.case_reference(case)[0]
    N, M = R.shape
    rng = np.random.default_rng(N + 3 * M + nv)
    h2 = max(float(np.mean(np.min(R, axis=1))) / X.shape[1], 1e-12)
    c = 1.0 / (2.0 * h2)
    w = rng.random(M) + 0.05
    a = np.full(M, -np.log(M)) if equal else np.log(w / w.sum())
    Y = 1.0 - rng.random((M, nv))
    b, lse, q = mixture_rows(R, a, c, Y)
    out = (R, a, c, Y, b, lse, q)
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------
class MixtureOracleBackend(dn.DensityOracleBackend):
    """DensityOracleBackend with ``mixture`` from the restatement on distortion.squared_matrix (TESTS ONLY); records the
    rows, the log-priors, c and Y of every call."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.mixture_calls = []

    def mixture(self, W, log_prior, c, Y, X):
        if hasattr(X, "toarray"):
            X = X.toarray()
        X = np.ascontiguousarray(X)
        assert not np.isnan(X).any() and len(X) > 0
        self.mixture_calls.append((len(X), np.array(log_prior), float(c), None if Y is None else np.array(Y)))
        b, lse, q = mixture_rows(ds.squared_matrix(X, W), log_prior, c, Y)
        return b, lse, (None if Y is None else q)
