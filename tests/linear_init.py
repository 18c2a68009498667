"""Helpers of the linear-initialisation tests (tests/test_linear_init_cpu.py, tests/test_gpu_linear_init.py).

- ``StandIn``: the CPU stand-in, ``OracleBackend`` with ``covariance_apply`` in NumPy -- rows centred in float64 exactly as
  csrc/covariance.hip centres them, then plain ``@``.
- ``exact``: the exact reference of one pass, the same centred C with every sum in ``np.longdouble`` (64-bit significand),
  and beside it the bound any float64 evaluation stays within, whatever its summation order, fused or not:
      |Z - Z_exact|[l, j] <= (N + d + 8) u sum_i |c_il| sum_k |c_ik| |V_kj|       |s - s_exact|[l] <= (N + 8) u sum_i |c_il|
  with u = 2^-53: y_ij is a sum of d products (d u, first order), Z_lj a sum of N products of c_il with it (N u), a few u
  for the partials' joins and the products' own roundings.  The reference's own error is the same expression with
  u_L = 2^-64, 2048 times smaller.
- ``planted``: a random rotation of independent columns with variances 16, 4, 0.25, ... plus an offset of several
  standard deviations.
- ``SHAPES``: the table of the raw kernel calls, and ``share`` / ``partials``: the launch geometry of covariance.hip restated,
  so that the CPU file can check that the table holds the rows it claims."""
import functools

import numpy as np

from oracle.som_oracle import OracleBackend

U = 2.0 ** -53
MAX_DIRECTIONS = 8
CV_R, CV_MAX_PARTIALS, CV_MIN_SHARE, CV_CHUNK = 4, 512, 64, 1024    # covariance.hip


def share(N):
    """rows per workgroup"""
    even = -(-(-(-N // CV_MAX_PARTIALS)) // CV_R) * CV_R
    return max(CV_MIN_SHARE, even)


def partials(N):
    return -(-N // share(N))


def centred(X, mean):
    """c_ik = widen(x_ik) - mean_k, rounded once in float64"""
    return np.asarray(X, dtype=np.float64) - np.asarray(mean, dtype=np.float64)[None, :]


class StandIn(OracleBackend):
    name = "oracle+covariance"

    def covariance_apply(self, mean, V):
        C = centred(self._X, mean)
        V = np.asarray(V, dtype=np.float64)
        return C.T @ (C @ V), C.sum(axis=0)


def exact(X, mean, V):
    """-> (Z, colsum, Z bound, colsum bound): the sums in np.longdouble, rounded to float64 at the end; the bounds of the
    module docstring (formed in np.longdouble as well, so that they are not themselves a rounding short)"""
    C = centred(X, mean).astype(np.longdouble)
    Vl = np.asarray(V, dtype=np.float64).astype(np.longdouble)
    N, d = C.shape
    Z = C.T @ (C @ Vl)
    s = C.sum(axis=0)
    A = np.abs(C)
    zb = (N + d + 8) * U * (A.T @ (A @ np.abs(Vl)))
    sb = (N + 8) * U * A.sum(axis=0)
    return Z, s, zb, sb


def within(got, want, bound):
    """every |got - want| <= bound, compared in np.longdouble -> (ok, worst ratio |err| / bound over entries with bound > 0)"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(np.longdouble) - want)
    ok = bool(np.all(err <= bound))
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return ok, worst


def planted(N, d, seed, dtype=np.float64, isotropic=False):
    """N x d rows: independent columns of variances 16, 4, 0.25, 0.25, ... (isotropic: all 1), rotated at random, plus an
    offset of several standard deviations per feature"""
    rng = np.random.default_rng(seed)
    var = np.full(d, 1.0 if isotropic else 0.25)
    if not isotropic:
        var[:2] = (16.0, 4.0)[:min(d, 2)]
    Y = rng.normal(size=(N, d)) * np.sqrt(var)[None, :]
    if d <= 1024:
        Y = Y @ np.linalg.qr(rng.normal(size=(d, d)))[0].T
    else:                                   # (wide rows: two random reflections, O(N d) instead of a d x d factorisation)
        for _ in range(2):
            u = rng.normal(size=d)
            u /= np.linalg.norm(u)
            Y = Y - 2.0 * np.outer(Y @ u, u)
    return np.ascontiguousarray(Y + rng.uniform(5.0, 20.0, size=d)[None, :], dtype=dtype)


def reference_spectrum(X):
    """-> (eigenvalues descending, eigenvectors as rows, signs fixed): np.linalg.eigh of the population covariance of X formed
    in np.longdouble"""
    Xl = np.asarray(X, dtype=np.float64).astype(np.longdouble)
    C = Xl - Xl.mean(axis=0)[None, :]
    cov = np.asarray((C.T @ C) / Xl.shape[0], dtype=np.float64)
    lam, E = np.linalg.eigh(cov)
    lam, E = lam[::-1], E[:, ::-1].T
    for e in E:
        if e[int(np.argmax(np.abs(e)))] < 0:
            e *= -1.0
    return lam, E


def direction_tolerance(lam, j):
    """4 * 1e-8 * l_1 / gap_j, gap_j the distance of l_j to its nearest other eigenvalue: Davis-Kahan for a residual of
    1e-8 l_1, with a factor 4 for the Ritz value's own error and eigh's rounding"""
    gap = np.abs(np.delete(lam, j) - lam[j]).min()
    return 4.0 * 1e-8 * lam[0] / gap


# (N, d, p, mean): N = 1; one row fewer / one more than a workgroup's share (64 rows up to N = 32768); several partials with
# an uneven last one, a multiple of the 4-row step (1000 = 15 * 64 + 40) and not (997 = 15 * 64 + 37); d = 1, 2, around one
# wave and one chunk of columns per thread (63, 64, 65; 256 / 257; 512 / 513), 785, the last width of the one-chunk form and
# the first of the chunked one (1024 / 1025), and 4099 (five chunks); p = 1, 2, 8; mean zeros / the true mean.
SHAPES = [
    (1, 1, 1, "zeros"), (1, 65, 8, "true"),
    (63, 2, 2, "true"), (63, 64, 8, "zeros"),
    (65, 63, 1, "true"), (65, 785, 8, "true"), (65, 4099, 1, "zeros"),
    (997, 1, 1, "true"), (997, 2, 1, "zeros"), (997, 65, 2, "zeros"), (997, 64, 2, "true"), (997, 63, 8, "zeros"),
    (997, 785, 8, "zeros"), (1000, 785, 2, "true"),
    (1000, 256, 8, "true"), (130, 257, 2, "zeros"), (130, 512, 8, "true"), (130, 513, 1, "true"),
    (129, 1024, 2, "zeros"), (129, 1025, 8, "true"), (300, 4099, 8, "true"),
    (20000, 64, 8, "true"),
]


@functools.lru_cache(maxsize=None)
def raw_case(N, d, p, mean_kind, dtype):
    """The inputs and the reference of one table line, made once: X (stored dtype), mean, V (any block, not orthonormal),
    and exact()'s four results."""
    X = planted(N, d, seed=7 * N + 3 * d + p, dtype=np.float32 if dtype == "f32" else np.float64)
    rng = np.random.default_rng(N + d + p)
    V = np.ascontiguousarray(rng.normal(size=(d, p)))
    mean = np.zeros(d) if mean_kind == "zeros" else np.asarray(X, dtype=np.float64).sum(axis=0) / N
    out = (X, mean, V) + exact(X, mean, V)
    for a in out:
        a.setflags(write=False)
    return out
