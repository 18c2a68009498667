"""Helpers of the row_neighbors tests (tests/test_row_neighbors_cpu.py, tests/test_gpu_row_neighbors.py): the restatement
of rho in NumPy, the oracle of the scan over probed cells (csrc/row_neighbors.hip), the tables of crafted buffers of the
raw call, and a CPU stand-in backend.

The contract (include/dbgsom_hip.h).  The rows X are filed under units: unit j's rows are order[seg_start[j] ..
seg_start[j + 1]).  The candidates of query q are the rows filed under the units probe[q] names (-1: skipped).  rho is
the direct-form squared distance in float64 in a fixed order (rho_rows); row q of the result holds the candidates with
the smallest (rho, i) in lexicographic order, dist = sqrt(rho); only rho < +inf is listed; the rest is (inf, -1)."""
import numpy as np

from tests import density as dn

MAX_NEIGHBORS = 32                    # DBGSOM_MAX_NEIGHBORS
MAX_SCAN_FEATURES = 8192              # DBGSOM_MAX_SCAN_FEATURES
K_INSTANCES = [1, 2, 4, 8, 16, 32]    # scan_cells_kernel<.., K>: the launcher takes the smallest K >= k
U = 2.0 ** -53


# ---- the restatement (the issue's, verbatim) ------------------------------------------------------------------------
def rho_rows(X, q):                      # X (n, d), q (d,), float32 or float64
    X, q = np.asarray(X, np.float64), np.asarray(q, np.float64)
    p = np.zeros((len(X), 64))
    for k0 in range(0, X.shape[1], 64):
        w = min(64, X.shape[1] - k0)
        t = X[:, k0:k0 + w] - q[k0:k0 + w]
        p[:, :w] = p[:, :w] + t * t
    for s in (32, 16, 8, 4, 2, 1):
        p = p + p[:, np.arange(64) ^ s]
    return p[:, 0]


def rho_bound(d):
    """relative error of rho_rows against the exact sum, in units of u = 2^-53: 3 for the rounded difference squared and
    rounded, ceil(d / 64) - 1 for the chain, 6 for the rounds, 1 of slack"""
    return (-(-d // 64) + 9) * U


# ---- oracle ---------------------------------------------------------------------------------------------------------
def oracle(X, winners, probes, Q, k):
    """-> (dist, idx), (len(Q), k): the candidate set from the winners and the probe lists, rho_rows, np.lexsort on
    (i, rho)"""
    X, Q = np.asarray(X), np.asarray(Q)
    winners, probes = np.asarray(winners), np.asarray(probes)
    dist, idx = np.full((len(Q), k), np.inf), np.full((len(Q), k), -1, dtype=np.int64)
    for qi in range(len(Q)):
        units = [u for u in probes[qi] if u >= 0]
        rows = np.flatnonzero(np.isin(winners, units))
        with np.errstate(all="ignore"):
            rho = rho_rows(X[rows], Q[qi])
        ok = rho < np.inf
        rows, rho = rows[ok], rho[ok]
        first = np.lexsort((rows, rho))[:k]
        idx[qi, :first.size] = rows[first]
        dist[qi, :first.size] = np.sqrt(rho[first])
    return dist, idx


def oracle_sorted_tuples(X, winners, probes, Q, k):
    """the same with a plain Python sort of (rho, i) tuples"""
    dist, idx = np.full((len(Q), k), np.inf), np.full((len(Q), k), -1, dtype=np.int64)
    for qi in range(len(Q)):
        units = {int(u) for u in probes[qi] if u >= 0}
        pairs = []
        for i in range(len(X)):
            if int(winners[i]) in units:
                with np.errstate(all="ignore"):
                    r = float(rho_rows(X[i:i + 1], Q[qi])[0])
                if r < float("inf"):
                    pairs.append((r, i))
        for t, (r, i) in enumerate(sorted(pairs)[:k]):
            dist[qi, t], idx[qi, t] = np.sqrt(r), i
    return dist, idx


def buckets(winners, M, descending=False):
    """-> (order int32, seg_start uint32 of M + 1): the stable bucket order of the rows by winner (rows whose winner is
    outside [0, M) are filed nowhere and come last); descending: the rows of a unit in falling order"""
    winners = np.asarray(winners, dtype=np.int64)
    filed = (winners >= 0) & (winners < M)
    key = np.where(filed, winners, M)
    order = np.argsort(key, kind="stable")
    seg = np.searchsorted(key[order], np.arange(M + 1)).astype(np.uint32)
    if descending:
        for j in range(M):
            order[seg[j]:seg[j + 1]] = order[seg[j]:seg[j + 1]][::-1]
    return order.astype(np.int32), seg


# ---- crafted buffers of dbgsom_ctx_scan_cells_device ----------------------------------------------------------------
SCAN_D = [1, 63, 64, 65, 129, 784, 8192]
SCAN_K = [1, 2, 5, 11, 31, 32]                       # 11 lies between the instances 8 and 16
# candidates of the query: both ends of the round-robin of four wavefronts over batches of 64, and of the unroll (eight
# rows in flight: 7, 8, 9; 3, 4, 5 are the ends of a narrower one)
SCAN_COUNTS = [0, 1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1025]
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]


def scan_case(seed, n_cand, d, k, xt=np.float32, qt=np.float32, M=7, n_probe=3, Nq=3, pad=0, descending=False):
    """A crafted problem whose FIRST query has exactly n_cand candidates -> dict(X, Q, winners, probes, order, seg, ...).
    X: n_cand rows under the units of query 0 and as many (at least 40) under the other units; values on a coarse grid
    so that equal rho abound; M units of which unit 1 is always empty (an empty cell between full ones); the probe
    list of query 0 holds a -1; the other queries probe random distinct units.  pad: X and Q are views of arrays with
    `pad` more columns of NaN (ldx, ldq > d)."""
    rng = np.random.default_rng(seed)
    others = max(40, n_cand)
    N = n_cand + others
    units0 = np.array([0, 2])                          # what query 0 probes (and a -1)
    rest = np.array([u for u in range(M) if u not in (0, 1, 2)])
    winners = np.concatenate([rng.choice(units0, n_cand), rng.choice(rest, others)])
    perm = rng.permutation(N)
    winners = winners[perm]
    Xf = np.round(rng.normal(size=(N, d + pad)) * 2) / 2
    Qf = np.round(rng.normal(size=(Nq, d + pad)) * 2) / 2
    if pad:
        Xf[:, d:] = np.nan
        Qf[:, d:] = np.nan
    Xf, Qf = Xf.astype(xt), Qf.astype(qt)
    X, Q = Xf[:, :d], Qf[:, :d]
    probes = np.empty((Nq, n_probe), dtype=np.int64)
    probes[0] = [0, -1, 2][:n_probe] if n_probe >= 3 else [0, 2][:n_probe]
    for qi in range(1, Nq):
        probes[qi] = rng.permutation(M)[:n_probe]
    order, seg = buckets(winners, M, descending)
    return dict(X=X, Q=Q, Xf=Xf, Qf=Qf, winners=winners, probes=probes, order=order, seg=seg, M=M, k=k, d=d)


def plant_specials(case):
    """Into a case with >= 256 candidates of query 0: duplicated rows in different wavefronts (batches of 64), lanes and
    cells, a row equal to the query, and rows with NaN, +inf and 1e200 (float64 X: rho overflows; float32 X cannot hold
    it and takes +inf) -- all among the candidates of query 0."""
    X, Q, order, seg, winners = case["X"], case["Q"], case["order"], case["seg"], case["winners"]
    c0 = order[seg[0]:seg[1]]            # cell of unit 0
    c2 = order[seg[2]:seg[3]]            # cell of unit 2
    cand = np.concatenate([c0, c2])      # positions of query 0's candidates in scan order
    assert len(cand) >= 256 and len(c0) >= 70 and len(c2) >= 3
    near = Q[0].astype(X.dtype)
    near[0] += X.dtype.type(0.5)
    # the same nearby row at positions 1 and 67 (wavefronts 0 and 1, lanes 1 and 3), 130 (wavefront 2) and in unit 2's cell
    for r in (cand[1], cand[67], cand[130], c2[-1]):
        X[r] = near
    X[cand[5]] = Q[0].astype(X.dtype)    # rho == 0 (exactly the query where the dtypes allow)
    X[cand[7], 0] = np.nan
    X[cand[8], 0] = np.inf
    X[cand[9], 0] = 1e200 if X.dtype == np.float64 else np.inf
    return case


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------
class RowNeighborsOracleBackend(dn.DensityOracleBackend):
    """DensityOracleBackend that counts its loads (``resident_serial``) and so can carry an index: ``partition`` and
    ``row_neighbors`` are HotPathBackend's NumPy defaults (TESTS ONLY)."""

    device_index = 0

    def load(self, X):
        self.resident_serial += 1
        return super().load(X)

    def release(self):
        self.resident_serial += 1
        return super().release()
