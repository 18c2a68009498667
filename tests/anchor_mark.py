"""The candidate rule of anchor_mark_kernel (csrc/filter.hip 2f) restated in NumPy with the code's margins, the run table
of launch_anchor_runs, and the inputs of tests/test_anchor_mark_cpu.py and tests/test_gpu_anchor_mark_device.py.

With a = the anchor of sample i, p = the anchor's seed and r_i >= |x_i - a|, prototype j is ruled out for i when
L[a][j] - U[a] >= 2 r_i + m_i, m_i = sqrt(2 rho_i).  Then |x_i - w_j|^2 >= |x_i - w_p|^2 + 2 rho_i: whatever is kept
includes every j with |x_i - w_j|^2 < min_j |x_i - w_j|^2 + 2 rho_i -- the winner, every tie partner and every
prototype the float64 chain could confuse with them.  `must_keep` states that set with np.longdouble distances."""
import zlib

import numpy as np

L = np.longdouble
U = 2.0 ** -53
R_MARGIN = 2.0 ** -52          # R = sqrt(sum) (1 + (d + 8) 2^-52)
GROUP = 128


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def long_above(M):
    return max(M // 8, 96)


# ---- the run table ----------------------------------------------------------------------------------------------------
def run_table(X, anchors, anchor_of, order, xx=None):
    """X: N x d values (float64 holds every storage type exactly), anchors A x d float64 -> dict run_start (nb + 1),
    anchor, R2 (np.longdouble: the largest exact squared distance of the run, inf where not finite), xx_max"""
    Xl, al = np.asarray(X, dtype=np.float64).astype(L), np.asarray(anchors, dtype=np.float64).astype(L)
    N = Xl.shape[0]
    if xx is None:
        xx = (np.asarray(X, dtype=np.float64) ** 2).sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = ((Xl - al[anchor_of]) ** 2).sum(axis=1)
    bad = ~(np.isfinite(r2.astype(np.float64)) & np.isfinite(xx))
    r2 = np.where(bad, L(np.inf), r2)
    xv = np.where(bad, np.inf, xx)
    start, anchor, R2, xm = [0], [], [], []
    for g0 in range(0, N, GROUP):
        pos = order[g0:g0 + GROUP]
        a = anchor_of[pos]
        heads = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
        for h, e in zip(heads, np.r_[heads[1:], len(a)]):
            anchor.append(int(a[h])); R2.append(r2[pos[h:e]].max()); xm.append(xv[pos[h:e]].max())
        start.append(len(anchor))
    return {"run_start": np.array(start, dtype=np.int32), "anchor": np.array(anchor, dtype=np.int32),
            "R2": np.array(R2, dtype=L), "xx_max": np.array(xm, dtype=np.float64)}


def widened_R(R2, d):
    """what the device stores for an exact squared radius, at the least and at the most: sqrt, the stated margin,
    and the (d + 2) roundings the margin covers on either side"""
    with np.errstate(invalid="ignore"):
        r = np.sqrt(R2.astype(L))
    lo = r
    hi = r * L(1.0 + 2.0 * (d + 8) * R_MARGIN)
    return lo, hi


# ---- the bounds anchor_seed_kernel keeps ------------------------------------------------------------------------------
def finite_rows(W):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(W).all(axis=1) & np.isfinite((W * W).sum(axis=1))


def f32_down(v):
    """float64 -> float32 rounded towards zero (v >= 0)"""
    f = v.astype(np.float32)
    over = f.astype(np.float64) > v
    return np.where(over, np.nextafter(f, np.float32(0)), f).astype(np.float32)


def bounds(anchors, W, d=None):
    """float64 restatement of alow / aup / aseed: -> (low A x M float32, up A float64, seed A)"""
    a, W = np.asarray(anchors, dtype=np.float64), np.asarray(W, dtype=np.float64)
    d = a.shape[1] if d is None else d
    with np.errstate(over="ignore", invalid="ignore"):
        aa, ww = (a * a).sum(axis=1), (W * W).sum(axis=1)
        v = ww[None, :] - 2.0 * (a @ W.T)
        yy_max = np.fmax.reduce(ww) if ww.size else 0.0
        rho_a = 4.0 * (d + 16) * U * (aa + yy_max)
        lo2 = ((aa[:, None] + v) - rho_a[:, None]) * (1.0 - 1e-12)
        ok = (lo2 > 0.0) & (lo2 < 3.0e38)
        low = np.where(ok, f32_down(np.where(ok, lo2, 1.0)), np.float32(0))
        key = np.where(np.isfinite(ww)[None, :], np.where(np.isfinite(v), v, np.finfo(np.float64).max), np.inf)
        seed = key.argmin(axis=1)
        bv = key[np.arange(a.shape[0]), seed]
        up2 = ((aa + bv) + rho_a) * (1.0 + 1e-12)
        up = np.where(up2 > 0.0, np.sqrt(np.maximum(up2, 0.0)) * (1.0 + 1e-12), 0.0)
        up = np.where((up2 == up2) & (up < np.inf), up, np.inf)
    return low, up, seed, yy_max


def rule_lists(table_R, table, low, up, seed, yy_max, M, d):
    """the lists of anchor_mark_kernel from a run table (table_R: the widened radii), before any hand-over:
    -> list of sorted index arrays, one per workgroup"""
    out = []
    rs = table["run_start"]
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(len(rs) - 1):
            keep = np.zeros(M, dtype=bool)
            whole = False
            for r in range(rs[g], rs[g + 1]):
                a = table["anchor"][r]
                rho = 4.0 * (d + 16) * U * (table["xx_max"][r] + yy_max)
                T = (up[a] + 2.0 * table_R[r]) * (1.0 + 1e-12) + np.sqrt(2.0 * rho) * 1.0001
                T2 = T * T * (1.0 + 1e-12)
                if not T2 < np.inf:
                    whole = True
                    break
                T2 = max(T2, np.finfo(np.float64).tiny)
                keep |= ~(low[a].astype(np.float64) >= T2)
                keep[seed[a]] = True
            out.append(np.arange(M) if whole else np.flatnonzero(keep))
    return out


# ---- what a list must hold --------------------------------------------------------------------------------------------
def exact_r(X, W):
    Xl, Wl = np.asarray(X, dtype=np.float64).astype(L), np.asarray(W, dtype=np.float64).astype(L)
    return ((Xl[:, None, :] - Wl[None, :, :]) ** 2).sum(axis=2) if X.shape[0] * W.shape[0] * X.shape[1] <= 4e6 else \
        (Xl ** 2).sum(1)[:, None] - 2 * (Xl @ np.ascontiguousarray(Wl.T)) + (Wl ** 2).sum(1)[None, :]


def must_keep(X, W, d=None, slack=0.0):
    """N x M bool: j with |x_i - w_j|^2 < min_j + (2 - slack) rho_i (np.longdouble distances -- `slack` 0.01 where
    exact_r takes the expanded form, whose own rounding is d 2^-64 (|x|^2 + |w|^2), a 2^-11-th of rho; rows of W that
    are not finite never count, a sample row that is not finite must keep every prototype)"""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    d = X.shape[1] if d is None else d
    fin = finite_rows(W)
    Wz = np.where(fin[:, None], W, 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        xx, ww = (X * X).sum(axis=1), (Wz * Wz).sum(axis=1)
        r = exact_r(np.where(np.isfinite(X), X, 0.0), Wz)
        r[:, ~fin] = np.inf
        rho = 4.0 * (d + 16) * U * (xx + (ww[fin].max() if fin.any() else 0.0))
        keep = r < (r.min(axis=1) + L(2.0 - slack) * rho.astype(L))[:, None]
    keep[~np.isfinite(xx)] = True
    return keep


def group_sets(keep, order):
    """per 128-sample workgroup of `order`: the union of its samples' rows of `keep`"""
    return [np.flatnonzero(keep[order[g0:g0 + GROUP]].any(axis=0)) for g0 in range(0, len(order), GROUP)]


# ---- inputs -----------------------------------------------------------------------------------------------------------
def blobs(N, d, M, key, radii=8.0, clusters=8):
    """clusters about `radii` cluster radii apart (unit noise: radius sqrt(d); centres radii / sqrt(2) times a normal
    vector: sqrt(d) radii apart on average), the map drawn from the samples"""
    rng = rng_for("blobs", N, d, M, key)
    centres = radii / np.sqrt(2.0) * rng.standard_normal((clusters, d))
    X = (centres[rng.integers(0, clusters, N)] + rng.standard_normal((N, d))).astype(np.float32)
    W = X[rng.choice(N, M, replace=M > N)].astype(np.float64) + 0.05 * rng.standard_normal((M, d))
    return X, np.ascontiguousarray(W)


def buckets(X, A, key=0):
    """anchors = A strided rows of X (float64), every sample at its nearest anchor, the stable bucket order"""
    N = X.shape[0]
    A = min(A, N)
    rows = (np.arange(A, dtype=np.int64) * N) // A
    anchors = np.ascontiguousarray(np.asarray(X, dtype=np.float64)[rows])
    if 2 < A < N:                    # (chain order, as the context numbers them: neighbouring buckets share a cluster)
        from tests import anchor_seeds

        anchors = np.ascontiguousarray(anchors[anchor_seeds.chain(np.nan_to_num(anchors))])
    if A == N:
        aof = np.arange(N, dtype=np.int32)
    else:
        Xd = np.nan_to_num(np.asarray(X, dtype=np.float64))
        ad = np.nan_to_num(anchors)
        r = (Xd ** 2).sum(1)[:, None] - 2 * Xd @ ad.T + (ad ** 2).sum(1)[None, :]
        aof = r.argmin(axis=1).astype(np.int32)
    return anchors, aof, np.argsort(aof, kind="stable").astype(np.int32)
