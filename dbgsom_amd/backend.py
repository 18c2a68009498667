"""Hot-path backends: the object the estimator calls once per epoch.

``HipBackend`` is a thin caller of the context level of the C ABI (``include/dbgsom_hip.h``,
``dbgsom_ctx_*``): NumPy arrays in, NumPy arrays out.  Everything else -- device memory, feature
padding, bfloat16 storage, digit planes, the choice of BMU search, previous winners as seeds,
device-resident prototypes -- lives behind that boundary in ``csrc/engine.hip`` (the policy of the filtered
search in ``csrc/search_policy.h``, host-only and replayable on the CPU).  PyTorch appears
in exactly one place: ``torch.distributed`` (backend ``nccl`` = RCCL over xGMI) supplies the one
all-reduce of the per-prototype sums per epoch, plugged into the context as a callback.  There is
no CPU fallback: constructing a ``HipBackend`` without the built library or without a GPU raises.

The four operations mirror the private methods of the reference's ``BaseSom``
(``dbgsom/BaseSom.py``):

    bmu(W, k)                    _get_winning_neurons(data, n_bmu)        :446-464
    exp_similarity(dist, gamma)  _calculate_exp_similarity(distances)     :533-538
    update(...)                  _update_weights(sample_weights, winners, data) :470-523
                                 + _write_accumulative_error              :541-561
    epoch(...)                   the fused body of _grow_som              :403-407
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native


@dataclass
class EpochResult:
    new_weights: np.ndarray      # (M, d) float64
    change_total: float          # sum_j |W_j - W'_j|_2
    errors: np.ndarray           # (M,) per-neuron sum of BMU distances
    activations: np.ndarray      # (M,) hit counts
    winners: Optional[np.ndarray] = None    # (N_local,) int64
    distances: Optional[np.ndarray] = None  # (N_local,) float64
    new_weights_dev: object = None          # device-resident copy (HipBackend, keep_on_device)
    class_hist: Optional[np.ndarray] = None  # (M, n_classes) int64 when labels were attached


def shard_bounds(n: int, rank: int, world: int):
    """Contiguous row shard [lo, hi) of rank `rank` (row-shard X once)."""
    return (n * rank) // world, (n * (rank + 1)) // world


def dist_info():
    """(rank, world) of the default process group, (0, 1) when torch.distributed is not up."""
    try:
        import torch.distributed as td

        if td.is_available() and td.is_initialized():
            return td.get_rank(), td.get_world_size()
    except ImportError:  # pragma: no cover
        pass
    return 0, 1


def _group_is_up() -> bool:
    try:
        import torch.distributed as td

        return td.is_available() and td.is_initialized()
    except ImportError:  # pragma: no cover
        return False


def squared_threshold(rho) -> float:
    """The largest float64 ``t`` with ``sqrt(t) <= rho`` under correctly rounded ``sqrt``, for a finite ``rho >= 0``:
    ``rho * rho`` stepped with ``nextafter`` until ``sqrt(t) <= rho < sqrt(nextafter(t, inf))``.  ``sqrt`` is monotone and
    correctly rounded on the host and on the device, so ``r <= t`` is exactly ``sqrt(r) <= rho`` for every ``r >= 0``:
    ``range_counts`` compares squared values and takes no root per pair.  (A ``rho`` whose square overflows gives the
    largest finite float64: no finite ``r`` has a root above it.)"""
    rho = float(rho)
    if not (np.isfinite(rho) and rho >= 0.0):
        raise ValueError(f"a radius must be finite and >= 0, got {rho!r}")
    big = float(np.finfo(np.float64).max)
    with np.errstate(over="ignore", under="ignore"):
        t = min(float(np.float64(rho) * np.float64(rho)), big)
    while np.sqrt(t) > rho:
        t = float(np.nextafter(t, -np.inf))
    while t < big and np.sqrt(np.nextafter(t, np.inf)) <= rho:
        t = float(np.nextafter(t, np.inf))
    return t


def squared_thresholds(radii) -> np.ndarray:
    """``squared_threshold`` of every radius, as a contiguous float64 vector"""
    return np.array([squared_threshold(r) for r in np.asarray(radii, dtype=np.float64).reshape(-1)], dtype=np.float64)


def _lane_sums(A) -> np.ndarray:
    """The row sums of A (rows x M float64) in the fixed order of the rows kernels (include/dbgsom_hip.h): lane l of 64
    adds its entries j = l, l + 64, ... ascending from +0.0, then six rounds m = 1 .. 32 in which every lane takes
    ``p_l + p_(l ^ m)``.  (A partial that starts at +0.0 is never -0.0, so the zeros that pad the last group of 64 change
    no bit.)"""
    n, M = A.shape
    G = -(-M // 64)
    P = np.zeros((n, G * 64))
    P[:, :M] = A
    P = P.reshape(n, G, 64)
    p = np.zeros((n, 64))
    for g in range(G):
        p = p + P[:, g]
    lanes = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        p = p + p[:, lanes ^ m]
    return p[:, 0]


def rho_rows(X, q) -> np.ndarray:
    """The direct-form squared distance of every row of X (n x d) to q (d,) in float64, bit for bit what
    csrc/row_neighbors.hip computes (include/dbgsom_hip.h): float32 values widened exactly; partial l of 64 takes the
    features l, l + 64, ... ascending with ``t = x_k - q_k``, ``p_l = p_l + t * t``, every operation rounded on its own;
    then six rounds ``p_l = p_l + p_(l ^ s)`` for s = 32, 16, 8, 4, 2, 1."""
    X, q = np.asarray(X, np.float64), np.asarray(q, np.float64)
    p = np.zeros((len(X), 64))
    with np.errstate(all="ignore"):
        for k0 in range(0, X.shape[1], 64):
            w = min(64, X.shape[1] - k0)
            t = X[:, k0:k0 + w] - q[k0:k0 + w]
            p[:, :w] = p[:, :w] + t * t
        for s in (32, 16, 8, 4, 2, 1):
            p = p + p[:, np.arange(64) ^ s]
    return p[:, 0]


def check_row_neighbors(k, n_probe, M) -> None:
    """The limits of ``row_neighbors``: rows listed per query and units probed per query"""
    if not 1 <= k <= _native.MAX_NEIGHBORS:
        raise ValueError(f"need 1 <= k <= DBGSOM_MAX_NEIGHBORS = {_native.MAX_NEIGHBORS}, got k = {k}")
    if not 1 <= n_probe <= min(M, _native.MAX_NEIGHBORS):
        raise ValueError(f"need 1 <= n_probe <= min({M} prototypes, DBGSOM_MAX_NEIGHBORS = {_native.MAX_NEIGHBORS}), "
                         f"got n_probe = {n_probe}")


def nearest_rows_host(X, winners, probes, Q, k):
    """The statement of ``row_neighbors`` in NumPy -> (dist, idx), both (rows of Q, k): the candidates of query q are
    the rows i of X whose unit ``winners[i]`` is among ``probes[q]`` (entries < 0 skipped); of those with
    ``rho_rows < +inf`` the k smallest ``(rho, i)`` in lexicographic order, ``dist = sqrt(rho)``; the rest ``(inf, -1)``."""
    X, Q = np.asarray(X), np.asarray(Q)
    winners, probes = np.asarray(winners, dtype=np.int64), np.asarray(probes, dtype=np.int64)
    dist, idx = np.full((len(Q), k), np.inf), np.full((len(Q), k), -1, dtype=np.int64)
    for qi in range(len(Q)):
        rows = np.flatnonzero(np.isin(winners, probes[qi][probes[qi] >= 0]))
        rho = rho_rows(X[rows], Q[qi])
        ok = rho < np.inf
        rows, rho = rows[ok], rho[ok]
        first = np.lexsort((rows, rho))[:k]
        idx[qi, :first.size], dist[qi, :first.size] = rows[first], np.sqrt(rho[first])
    return dist, idx


def mixture_rows_host(R, log_prior, c, Y=None):
    """The arithmetic of csrc/mixture.hip in NumPy on a matrix R (rows x M float64) of squared values -> (unit, lse, q):
    ``t_j = a_j - (c * r_j)``, two roundings; ``(T, b)`` the largest t_j, lowest j among equals, over ``t_j > -inf`` and
    not NaN; ``s_j = exp(t_j - T)``; ``S = sum_j s_j`` and ``Q_v = sum_j (s_j * Y[j, v])`` in the order of ``_lane_sums``;
    ``lse = T + log(S)``, ``q_v = Q_v / S``.  A NaN t_j enters the sums as it is; a row without any t_j above -inf has
    ``(-1, NaN, NaN)``.  ``Y`` None: q is None.  What differs from the device is the library behind exp and log."""
    R = np.asarray(R, dtype=np.float64)
    a = np.asarray(log_prior, dtype=np.float64).reshape(-1)
    n = R.shape[0]
    with np.errstate(all="ignore"):
        t = a[None, :] - (np.float64(c) * R)
        ok = t > -np.inf
        has = ok.any(axis=1)
        b = np.argmax(np.where(ok, t, -np.inf), axis=1)     # the first maximum: the lowest index
        T = t[np.arange(n), b]
        s = np.exp(t - T[:, None])
        S = _lane_sums(s)
        lse = np.where(has, T + np.log(S), np.nan)
        q = None
        if Y is not None:
            Y = np.asarray(Y, dtype=np.float64)
            q = np.stack([_lane_sums(s * Y[None, :, v]) / S for v in range(Y.shape[1])], axis=1).reshape(n, Y.shape[1])
            q[~has] = np.nan
    return np.where(has, b, -1).astype(np.int64), lse, q


def _mixture_args(M, log_prior, c, Y):
    """-> (a (M,) float64, c as a float, Y (M, V) float64 or None) for ``mixture``, checked"""
    a = np.ascontiguousarray(log_prior, dtype=np.float64)
    if a.shape != (M,):
        raise ValueError(f"log_prior must be ({M},), one value per prototype, got {a.shape}")
    c = float(c)
    if not c >= 0.0:
        raise ValueError(f"c must be >= 0, got {c!r}")
    if Y is not None:
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[0] != M:
            raise ValueError(f"Y must be ({M}, n_values), one row per prototype, got {Y.shape}")
        if not 1 <= Y.shape[1] <= _native.MAX_MIXTURE_VALUES:
            raise ValueError(f"need 1 .. DBGSOM_MAX_MIXTURE_VALUES = {_native.MAX_MIXTURE_VALUES} values per prototype, "
                             f"got {Y.shape[1]}")
    return a, c, Y


UNIT_BLOCK = 128          # list positions per block of the per-unit sums: CH of csrc/accumulate.hip
DEVIATIONS_SQUARES, DEVIATIONS_NORM = _native.DEVIATIONS_SQUARES, _native.DEVIATIONS_NORM


def _unit_args(units, Y, w):
    units = np.ascontiguousarray(units, dtype=np.int64).reshape(-1)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    if Y.ndim != 2 or Y.shape[0] != units.shape[0]:
        raise ValueError("one row of values per unit index")
    if not 1 <= Y.shape[1] <= _native.MAX_MIXTURE_VALUES:
        raise ValueError(f"1 .. {_native.MAX_MIXTURE_VALUES} values per row, got {Y.shape[1]}")
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if w.shape != units.shape:
            raise ValueError("one weight per row")
    return units, Y, w


def unit_fold(units, Z, w, M):
    """The per-unit sums of csrc/unit_sums.hip in NumPy, bit for bit -> (mass (M,), sums (M, V)).

    The list of unit j holds the rows i with ``units[i] == j``, ascending, without rows of weight 0; a row's term is
    ``Z[i, v]`` or the rounded product ``w[i] * Z[i, v]``, its mass term 1.0 or ``w[i]``.  The list is cut into
    blocks of UNIT_BLOCK positions, a block's terms are added in list order from +0.0, and the blocks' partial sums
    are added ascending from +0.0 (``np.add.accumulate`` is sequential).  A block is padded with +0.0 here: adding
    +0.0 to a chain that started at +0.0 changes no bit."""
    units, Z = np.asarray(units, dtype=np.int64), np.asarray(Z, dtype=np.float64)
    N, V = Z.shape
    M = int(M)
    keep = (units >= 0) & (units < M)
    if w is not None:
        keep &= np.asarray(w) != 0
    rows = np.flatnonzero(keep)
    order = rows[np.argsort(units[rows], kind="stable")]
    counts = np.bincount(units[order], minlength=M)
    seg = np.concatenate([[0], np.cumsum(counts)])
    nblk = -(-counts // UNIT_BLOCK)
    pre = np.concatenate([[0], np.cumsum(nblk)])
    B = int(pre[-1])
    of = np.repeat(np.arange(M), nblk)
    start = seg[of] + UNIT_BLOCK * (np.arange(B) - pre[of])
    end = np.minimum(start + UNIT_BLOCK, seg[of + 1])
    P = np.zeros((B, V + 1))
    with np.errstate(all="ignore"):
        for b0 in range(0, B, 1024):
            b1 = min(B, b0 + 1024)
            pos = start[b0:b1, None] + np.arange(UNIT_BLOCK)[None, :]
            ok = pos < end[b0:b1, None]
            r = order[np.where(ok, pos, 0)]
            T = np.zeros((b1 - b0, UNIT_BLOCK + 1, V + 1))
            if w is None:
                zt, mt = Z[r], np.ones(r.shape)
            else:
                mt = w[r]
                zt = mt[..., None] * Z[r]
            T[:, 1:, :V] = np.where(ok[..., None], zt, 0.0)
            T[:, 1:, V] = np.where(ok, mt, 0.0)
            P[b0:b1] = np.add.accumulate(T, axis=1)[:, -1]
        out = np.zeros((M, V + 1))
        for j in np.flatnonzero(nblk):
            out[j] = np.add.accumulate(np.concatenate([np.zeros((1, V + 1)), P[pre[j]:pre[j + 1]]]), axis=0)[-1]
    return np.ascontiguousarray(out[:, V]), np.ascontiguousarray(out[:, :V])


def unit_deviations(units, Y, C, mode):
    """Row i with unit j inside [0, len(C)): ``(Y[i, v] - C[j, v])^2`` (N x V) under DEVIATIONS_SQUARES, the root of
    their sum over v ascending from +0.0 (N,) under DEVIATIONS_NORM; +0.0 for the other rows."""
    units, Y, C = np.asarray(units, dtype=np.int64), np.asarray(Y, dtype=np.float64), np.asarray(C, dtype=np.float64)
    inside = (units >= 0) & (units < len(C))
    with np.errstate(all="ignore"):
        df = Y - C[np.where(inside, units, 0)]
        sq = df * df
        if mode == DEVIATIONS_SQUARES:
            return np.where(inside[:, None], sq, 0.0)
        s = np.zeros(len(units))
        for v in range(Y.shape[1]):
            s = s + sq[:, v]
        return np.where(inside, np.sqrt(s), 0.0)


class HotPathBackend:
    """Epoch template shared by the HIP backend and the test-only oracle backend:
    local per-prototype sums -> (all-reduce across sample shards) -> smoothing.

    ``load(X)`` and ``bmu(W, k, X=...)`` may be handed a scipy sparse matrix in CSR form (the estimators
    pass sparse input through as it is); every other argument is dense.

    A backend that can adopt rows living in GPU memory (``is_device_array``) has ``load_device(X)`` and takes such
    an X in ``bmu``, ``sparse_code`` and ``topographic_function``; per-row results then come back as arrays next
    to X.  ``device_index`` is the GPU it runs on."""

    name = "abstract"

    # -- to implement -------------------------------------------------------------------------
    def load(self, X):  # upload-once residency
        raise NotImplementedError

    def bmu(self, W, k=1, X=None):
        raise NotImplementedError

    def bmu_masked(self, W, k, X, want_filled=False):
        """``bmu(W, k, X=X)`` for dense rows with missing entries (NaN): the distance of a row x to a prototype w
        is ``sqrt(d / n_obs * sum over the observed entries of (x - w) ** 2)`` in float64, direct form
        (scikit-learn's ``nan_euclidean_distances``); ties go to the lowest index.  -> (distances, winners) in
        ``bmu``'s shapes, and with ``want_filled`` a copy of X with every hole filled from the row's first winner."""
        raise NotImplementedError

    def distances(self, W, X):
        """The (rows of X, rows of W) float64 matrix of distances in the arithmetic of ``bmu(W, k, X=X)``, bit for
        bit -- ``bmu``'s distances are its smallest entries per row.  X: a dense host array, a scipy sparse matrix
        or (a backend that takes them) a device array; the result is a NumPy array, next to X for a device array."""
        raise NotImplementedError

    def distances_masked(self, W, X):
        """``distances(W, X)`` for dense host rows with missing entries (NaN), in the arithmetic of ``bmu_masked``."""
        raise NotImplementedError

    def kneighbors(self, W, k, X):
        """The k rows of W nearest to every row of X -> (distances, indices), both (rows of X, k), float64 and
        int64: the k smallest ``(r, j)`` per row in lexicographic order, ascending, r the squared value of
        ``bmu(W, k, X=X)``'s arithmetic and the distance its square root -- ``distances(W, X)`` gathered at the
        indices, bit for bit.  Slots without a pair below +inf hold (inf, -1).  X as for ``distances``; the results
        are NumPy arrays, next to X for a device array."""
        raise NotImplementedError

    def kneighbors_masked(self, W, k, X):
        """``kneighbors(W, k, X)`` for dense host rows with missing entries (NaN), in the arithmetic of
        ``bmu_masked``."""
        raise NotImplementedError

    def neighborhood_energy(self, W, H, X):
        """The distortion measure of every row of X -> (e, bmu), both (rows of X,), float64 and int64: ``bmu`` is the
        index of the smallest ``(r, j)`` in lexicographic order among ``r < inf``, r the squared value of
        ``bmu(W, k, X=X)``'s arithmetic (``kneighbors``' first index), and ``e = sum_j H[bmu, j] * r_j`` with H the
        (rows of W, rows of W) float64 neighbourhood factors.  The order of the sum is fixed (include/dbgsom_hip.h):
        64 strided partials of rounded products, ascending, then six xor rounds.  A row without an ``r`` below +inf
        has (NaN, -1).  X as for ``distances``; the results are NumPy arrays, next to X for a device array."""
        raise NotImplementedError

    def exemplars(self, W, k, X, own_cell=False):
        """The k nearest rows of X to every prototype -> (dist, idx), both (rows of W, k), float64 and int64: row ``j``
        holds the rows of X with the smallest ``(r_ij, i)`` in lexicographic order, ascending, r the squared value of
        ``bmu(W, k, X=X)``'s arithmetic (what ``kneighbors`` selects on), ``dist = sqrt(r)`` taken after the selection
        and ``idx`` row numbers of X.  Equal r go by the lower row; a pair whose r is not below +inf is never
        reported; slots left unfilled hold ``(inf, -1)`` (k may exceed the rows of X, 1 <= k <= MAX_NEIGHBORS).
        ``own_cell``: row ``i`` is a candidate for prototype ``j`` only if ``j`` is the row's unit, the index of its
        smallest ``(r_ij, j)`` (``kneighbors(W, 1, X)``); a row without an r below +inf belongs to no unit.  ``(r, i)``
        is a total order: the result does not depend on chunks or slabs.  X as for ``distances``; the results are
        NumPy arrays, next to X for a device array."""
        raise NotImplementedError

    def range_counts(self, W, thresholds_squared, X):
        """The rows of X within a radius of every prototype -> counts, (rows of W, thresholds) int64:
        ``counts[j, t] = #{ i : r_ij <= thresholds_squared[t] }``, r the squared value of ``bmu(W, k, X=X)``'s
        arithmetic (what ``kneighbors`` selects on); 1 .. MAX_RADII thresholds in any order.  A pair whose r is NaN
        is never counted.  Integer counts: the result does not depend on chunks or slabs.  X as for ``distances``; the
        result is a NumPy array, next to X for a device array.

        This default counts on the host over ``distances(W, X)``, whose entries are ``sqrt(r)``: it is exact for the
        thresholds ``squared_threshold`` makes, the largest t under their root, for which ``sqrt(r) <= sqrt(t)`` is
        ``r <= t``.  The HIP backend compares squared values on the device and holds no N x M matrix."""
        thr = np.ascontiguousarray(thresholds_squared, dtype=np.float64).reshape(-1)
        if not 1 <= thr.size <= _native.MAX_RADII:
            raise ValueError(f"need 1 .. DBGSOM_MAX_RADII = {_native.MAX_RADII} thresholds, got {thr.size}")
        D = self.distances(W, X)
        D = D if isinstance(D, np.ndarray) else D.cpu().numpy()
        with np.errstate(invalid="ignore"):
            rho = np.sqrt(thr)
            return np.stack([np.count_nonzero(D <= r, axis=0) for r in rho], axis=1).astype(np.int64)

    # goes up whenever the resident rows are replaced or dropped (a backend that keeps a count: HipBackend): what an
    # index of the resident rows is held against
    resident_serial = 0

    def partition(self, W, want_winners=False):
        """The resident rows bucketed by their unit, ``bmu(W, 1)``'s winner -> (rows per unit (rows of W,) int64, the
        winners or None).  The partition stays with the backend until the resident rows change: ``row_neighbors``
        searches it.  This default keeps the winners on the host."""
        win = np.asarray(self.bmu(W, 1)[1], dtype=np.int64).reshape(-1)
        self._partition = (self.resident_serial, len(np.asarray(W)), win)
        counts = np.bincount(win, minlength=len(np.asarray(W))).astype(np.int64)
        return counts, (win if want_winners else None)

    def _resident_rows(self) -> np.ndarray:
        """The resident rows on the host, for the NumPy defaults."""
        X = getattr(self, "_X", None)
        if X is None:
            raise ValueError("no resident rows: call load(X) first")
        return X.toarray() if is_sparse(X) else np.asarray(X)

    def row_neighbors(self, W, k, n_probe, Q):
        """The k nearest resident rows of every row of Q among the rows filed under its n_probe nearest units ->
        (dist, idx), both (rows of Q, k), float64 and int64 (row numbers of the resident rows).  The units of row q
        are ``kneighbors(W, n_probe, Q)``'s indices (-1 skipped), its candidates the resident rows whose unit under
        the last ``partition`` is among them, and the result the candidates with the smallest ``(rho, i)`` in
        lexicographic order, ascending, ``rho = rho_rows`` (direct form, float64, fixed order) and ``dist =
        sqrt(rho)`` taken after the selection.  Only ``rho < +inf`` is listed; unfilled slots hold ``(inf, -1)``.
        ``1 <= k <= MAX_NEIGHBORS``, ``1 <= n_probe <= min(rows of W, MAX_NEIGHBORS)``.  ``ValueError`` without a
        partition of the rows that are resident now, on these many units.  Q: a dense host array or (a backend that
        takes them) a device array; the results are NumPy arrays, next to Q for a device array.

        This default is the statement of the semantics in NumPy (``nearest_rows_host``); the HIP backend scans the
        probed cells on the device (csrc/row_neighbors.hip)."""
        M = len(np.asarray(W))
        k, n_probe = int(k), int(n_probe)
        check_row_neighbors(k, n_probe, M)
        part = getattr(self, "_partition", None)
        if part is None or part[0] != self.resident_serial or part[1] != M:
            raise ValueError("no partition of the resident rows on these prototypes: call partition(W) after load(X)")
        if is_sparse(Q):
            raise TypeError("the row_neighbors calls take dense rows")
        Q = host_rows(Q)
        probes = np.asarray(self.kneighbors(W, n_probe, Q)[1]) if len(Q) else np.empty((0, n_probe), dtype=np.int64)
        return nearest_rows_host(self._resident_rows(), part[2], probes, Q, k)

    def mixture(self, W, log_prior, c, Y, X):
        """The map as an isotropic Gaussian mixture -> (unit, lse, q): (rows of X,) int64, (rows of X,) float64 and
        (rows of X, n_values) float64, or None for ``Y`` None.  With r the squared value of ``bmu(W, k, X=X)``'s
        arithmetic (what ``kneighbors`` selects on), ``log_prior`` (rows of W,) float64 (``-inf`` allowed), ``c = 1 /
        (2 h^2) >= 0`` and ``Y`` (rows of W, 1 .. MAX_MIXTURE_VALUES) float64: ``t_j = log_prior_j - c r_j``, ``unit``
        the index of the largest t_j (lowest among equals), ``lse = log sum_j exp(t_j)`` and ``q_v = sum_j exp(t_j) Y[j,
        v] / sum_j exp(t_j)``, evaluated as ``mixture_rows_host`` states it: the roundings and the order of the sums are
        fixed (include/dbgsom_hip.h).  A row without a t_j above -inf has (-1, NaN, NaN).  X as for ``distances``; the
        results are NumPy arrays, next to X for a device array.

        This default evaluates ``mixture_rows_host`` on the squares of ``distances(W, X)``, 4096 rows at a time: the
        square of a correctly rounded root is r to within two roundings, not r itself.  The HIP backend reads r on the
        device and holds no N x M matrix."""
        M = len(np.asarray(W))
        a, c, Y = _mixture_args(M, log_prior, c, Y)
        D = self.distances(W, X)
        D = D if isinstance(D, np.ndarray) else D.cpu().numpy()
        n = D.shape[0]
        unit, lse = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float64)
        q = None if Y is None else np.empty((n, Y.shape[1]), dtype=np.float64)
        for r0 in range(0, n, 4096):
            sl = slice(r0, min(n, r0 + 4096))
            with np.errstate(over="ignore", invalid="ignore"):
                R = D[sl] * D[sl]
            res = mixture_rows_host(R, a, c, Y)
            unit[sl], lse[sl] = res[0], res[1]
            if q is not None:
                q[sl] = res[2]
        return unit, lse, q

    def geodesics(self, W, edges):
        """The weighted geodesics of the lattice -> G, (rows of W, rows of W) float64.  ``edges`` is an (E, 2) integer
        array of undirected lattice edges, indices into the rows of W.  An edge is as long as its two prototypes are
        apart: ``len(a, b) = sqrt(s)`` with ``s = 0`` and then, k ascending, ``t = W[a, k] - W[b, k]``, ``p = t * t``,
        ``s = s + p``, each operation rounded on its own in float64 (no fma), so ``len(a, b) == len(b, a)`` bit for
        bit.  ``G[s, t]`` is the minimum over lattice paths ``s = v0, .., vn = t`` of the left fold ``((0 + len(v0,
        v1)) + len(v1, v2)) + ...``; ``G[s, s] = 0`` and ``G[s, t] = +inf`` without a path.  Rounded addition of a
        non-negative length is monotone, so the minimum is the unique least fixed point of ``dist[v] = min(dist[v],
        dist[u] + len(u, v))`` from ``dist[s] = 0`` and every relaxation order ends in the same bits.  ``G[s, t]`` and
        ``G[t, s]`` fold from different ends and differ in their last bits for most pairs: row s is the fold from s,
        nothing is symmetrised.  Self-loops are ignored, repeated edges are harmless."""
        raise NotImplementedError

    def combined_error(self, W, edges, X):
        """The combined error of Kaski and Lagus (1996) of every row of X -> (e, units), (rows of X,) float64 and
        (rows of X, 2) int64: ``units[i] = (b1, b2)`` and ``(d1, d2)`` are the first and second result of
        ``bmu(W, 2, X=X)``'s arithmetic without float32 rounding (ties to the lower index), and ``e_i = d1_i +
        G[b1_i, b2_i]``, one rounded addition, G as in ``geodesics(W, edges)``.  A row with index -1 in either slot
        has NaN; ``+inf`` when the two units lie in different components.  X as for ``distances``; the results are
        NumPy arrays, next to X for a device array."""
        raise NotImplementedError

    def covariance_apply(self, mean, V):
        """One pass over the resident rows for the linear initialisation (``dbgsom_amd.linear_init``): with
        ``C = X - mean`` (rows widened to float64, the difference rounded once) -> ``(Z, colsum)``, ``Z = C^T (C V)``
        of V's shape (d, p), 1 <= p <= MAX_DIRECTIONS, and ``colsum = sum_i C_i`` (d,), all float64.  Dense complete
        float32 / float64 rows, no weights, one rank.  A backend without it raises: no quiet fallback."""
        raise NotImplementedError(f"the {self.name} backend has no covariance_apply")

    # -- metric="manhattan": dist(x, w) = sum_k |x_k - w_k| in float64, k ascending, one accumulator per pair; float32
    # rows widened exactly first; no square root, no clamp; winners by (dist, index); a pair whose distance is not
    # below +inf is never reported (index -1, distance inf).  X: a dense host array or a device array.
    _metric = "euclidean"

    def set_metric(self, metric):
        """The metric of the search of the RESIDENT rows from here to the next ``load`` / ``release``: "euclidean",
        or "manhattan" -- ``bmu(W, k)`` is then the L1 search, ``epoch_manhattan`` the epoch, and the reductions over
        the resident rows are the host defaults of this class over that ``bmu`` -- or "cosine", likewise with the
        cosine search and ``epoch_cosine``."""
        if metric not in ("euclidean", "manhattan", "cosine"):
            raise ValueError(f"metric must be 'euclidean', 'manhattan' or 'cosine', got {metric!r}")
        self._metric = metric

    def bmu_manhattan(self, W, k, X):
        """``bmu(W, k, X=X)`` under the Manhattan metric -> (distances, winners) in ``bmu``'s shapes."""
        raise NotImplementedError

    def distances_manhattan(self, W, X):
        """``distances(W, X)`` under the Manhattan metric: ``bmu_manhattan``'s distances are its smallest entries."""
        raise NotImplementedError

    def kneighbors_manhattan(self, W, k, X):
        """``kneighbors(W, k, X)`` under the Manhattan metric: the k smallest ``(dist, j)`` per row, ascending;
        ``distances_manhattan(W, X)`` gathered at the indices, bit for bit."""
        raise NotImplementedError

    def epoch_manhattan(self, W, hop, sigma, gamma, layout="compact", want_assignments=False, n_classes=0):
        """``epoch`` with the L1 search in front of the unchanged sums and smoothing -> EpochResult.  The prototypes
        are handed over with every call."""
        raise NotImplementedError

    # -- metric="cosine": c(x, w) = 1 - (<x, w> * inv(|x|^2)) * inv(|w|^2) in float64, every operation rounded on its
    # own, clamped to [0, 2]; <x, w>, |x|^2, |w|^2 the sequential fma chains of ``bmu``; inv(t) = 0 for t == 0,
    # 1 / sqrt(t) for 0 < t < inf, NaN otherwise; no square root of c; winners by (c, index); a pair whose c is not below
    # +inf is never reported (index -1, distance inf).  X: a dense host array or a device array.
    def bmu_cosine(self, W, k, X):
        """``bmu(W, k, X=X)`` under the cosine metric -> (distances, winners) in ``bmu``'s shapes."""
        raise NotImplementedError

    def distances_cosine(self, W, X):
        """``distances(W, X)`` under the cosine metric: ``bmu_cosine``'s distances are its smallest entries."""
        raise NotImplementedError

    def kneighbors_cosine(self, W, k, X):
        """``kneighbors(W, k, X)`` under the cosine metric: the k smallest ``(c, j)`` per row, ascending;
        ``distances_cosine(W, X)`` gathered at the indices, bit for bit."""
        raise NotImplementedError

    def epoch_cosine(self, W, hop, sigma, gamma, layout="compact", want_assignments=False, n_classes=0):
        """``epoch`` with the cosine search in front of the unchanged sums and smoothing -> EpochResult.  The
        prototypes are handed over with every call."""
        raise NotImplementedError

    def exp_similarity(self, distances, gamma):
        raise NotImplementedError

    def _local_sums(self, W, gamma, want_assignments):
        """-> (sums tensor [M*(d+3)] float64 = [S | K | a | E], winners, distances)"""
        raise NotImplementedError

    def _sums_from(self, W, sample_weights, winners, distances):
        raise NotImplementedError

    def _smooth(self, sums, W, hop, sigma, layout):
        """-> (new_weights ndarray, change_total float, errors ndarray, activations ndarray)"""
        raise NotImplementedError

    # -- shared -------------------------------------------------------------------------------
    def _all_reduce(self, sums):
        rank, world = dist_info()
        # DBGSOM_FORCE_COLLECTIVE=1: issue the collective even in a 1-rank group (rehearsal of
        # the RCCL path on a single-GPU box)
        force = os.environ.get("DBGSOM_FORCE_COLLECTIVE") == "1"
        if world > 1 or (force and _group_is_up()):
            import torch.distributed as td

            td.all_reduce(sums, op=td.ReduceOp.SUM)  # one collective per epoch
        return sums

    def epoch(self, W, hop, sigma, gamma, layout="compact", want_assignments=False,
              n_classes=0):
        sums, win, dist = self._local_sums(W, gamma, want_assignments or n_classes > 0)
        sums = self._all_reduce(sums)
        Wn, chg, E, a = self._smooth(sums, W, hop, sigma, layout)
        res = EpochResult(Wn, chg, E, a, win if want_assignments else None,
                          dist if want_assignments else None)
        if n_classes > 0:
            res.class_hist = self.class_histogram(win, n_classes, np.asarray(W).shape[0])
        return res

    def update(self, W, hop, sigma, sample_weights, winners, distances, layout="compact"):
        sums = self._sums_from(W, sample_weights, winners, distances)
        sums = self._all_reduce(sums)
        return self._smooth(sums, W, hop, sigma, layout)

    def epoch_masked(self, W, hop, sigma, gamma, want_assignments=False, n_classes=0):
        """``epoch`` on resident rows with missing entries (``load(X, incomplete=True)``): the search of
        ``bmu_masked`` for every row, sums per (neuron, feature) over the rows that observe the feature, and a
        smoothing with a denominator per (neuron, feature) -- always the aligned form; an entry nobody in reach
        observed keeps its value.  -> EpochResult.  The prototypes are handed over with every call."""
        raise NotImplementedError

    # -- post-fit consumers of the BMU step; host defaults ----------
    def _reduce_host(self, arr):
        """Sum a small host array over the ranks (identity for one process)."""
        rank, world = dist_info()
        if world == 1:
            return arr
        import torch

        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64).copy())
        return self._all_reduce(t).numpy()

    def set_labels(self, y):
        """Attach integer class labels of the resident rows (entropy criterion)."""
        self._y = None if y is None else np.ascontiguousarray(y, dtype=np.int32)

    def set_sample_weight(self, w):
        """Attach one weight per resident row (``fit(..., sample_weight=w)``: a row of weight w counts
        as w copies of that row; None detaches).  The epoch sums and the reductions below are then the
        weighted ones: S = sum w h x, K = sum w h, a = sum w, E = sum w dist."""
        self._sw = None if w is None else np.ascontiguousarray(w, dtype=np.float64)

    _sw = None

    def quantization_error(self, W) -> float:
        dist, _ = self.bmu(W, 1)
        if self._sw is not None:
            s = self._reduce_host(np.array([self._sw @ dist, self._sw.sum()], dtype=np.float64))
            return float(s[0] / s[1])
        s = self._reduce_host(np.array([dist.sum(), dist.size], dtype=np.float64))
        return float(s[0] / s[1])

    def topographic_error_count(self, W, coords):
        """Rows whose two best matching units are not lattice neighbours: their number, or with
        weights attached their summed weight (a float)."""
        _, idx = self.bmu(W, 2)
        pos = np.asarray(coords, dtype=np.float64)
        apart = np.linalg.norm(pos[idx[:, 0]] - pos[idx[:, 1]], axis=1) > 1.5
        if self._sw is not None:
            return float(self._reduce_host(np.array([self._sw[apart].sum()], np.float64))[0])
        return int(round(self._reduce_host(np.array([np.count_nonzero(apart)], np.float64))[0]))

    def node_statistics(self, W, sigma):
        """-> (hit_counts (M,), density_sums (M,)) of BaseSom._calculate_node_statistics."""
        dist, win = self.bmu(W, 1)
        m = np.asarray(W).shape[0]
        terms = np.exp(-(dist ** 2) / (2 * sigma ** 2)) / (sigma * np.sqrt(2 * np.pi))
        if self._sw is not None:
            both = np.concatenate([np.bincount(win, weights=self._sw, minlength=m),
                                   np.bincount(win, weights=self._sw * terms, minlength=m)])
        else:
            both = np.concatenate([np.bincount(win, minlength=m).astype(np.float64),
                                   np.bincount(win, weights=terms, minlength=m)])
        both = self._reduce_host(both)
        return both[:m], both[m:]

    def class_histogram(self, winners, n_classes, M):
        """(M, n_classes) class counts per neuron over all ranks: int64, or with weights attached the
        summed weights (float64)."""
        h = np.zeros((M, n_classes), dtype=np.float64)
        np.add.at(h, (winners, self._y), 1.0 if self._sw is None else self._sw)
        h = self._reduce_host(h.reshape(-1)).reshape(M, n_classes)
        return h if self._sw is not None else h.astype(np.int64)

    # -- per-unit statistics of a per-row quantity (BaseSom.unit_means, SomRegressor); host default ------
    def unit_statistics(self, units, Y, w, M, want_std=False, want_err=False):
        """Per-unit statistics of the rows Y (N x V float64) filed under ``units`` (N int64; entries outside
        [0, M) are skipped), with weights w (N float64) or None -> (mass (M,), mean (M, V), std (M, V) | None,
        err (M,) | None): ``mean = sums / mass`` (NaN for a unit without mass), ``std = sqrt(fold((y - mean)^2) /
        mass)``, ``err = fold(||y - mean||_2)``, every fold in the order of ``unit_fold``.  This NumPy default is
        the restatement of csrc/unit_sums.hip."""
        units, Y, w = _unit_args(units, Y, w)
        mass, sums = unit_fold(units, Y, w, M)
        with np.errstate(all="ignore"):
            mean = sums / mass[:, None]
            std = err = None
            if want_std:
                m2, sq = unit_fold(units, unit_deviations(units, Y, mean, DEVIATIONS_SQUARES), w, M)
                std = np.sqrt(sq / m2[:, None])
            if want_err:
                err = unit_fold(units, unit_deviations(units, Y, mean, DEVIATIONS_NORM)[:, None], w, M)[1][:, 0]
        return mass, mean, std, err

    _targets = None

    def set_targets(self, Y):
        """Attach float64 targets (N x V) of the resident rows (growth_criterion="target_error"); None detaches."""
        self._targets = None if Y is None else np.ascontiguousarray(Y, dtype=np.float64).reshape(len(Y), -1)

    def target_statistics(self, winners, M, want_std=False, want_err=False):
        """``unit_statistics`` of the attached targets under the attached sample weights; one process only."""
        if dist_info()[1] > 1:
            raise ValueError("target statistics take one process")
        if self._targets is None:
            raise RuntimeError("no targets attached: call set_targets(Y) first")
        return HotPathBackend.unit_statistics(self, winners, self._targets, self._sw, M, want_std, want_err)

    # -- sparse coding (BaseSom.transform, SomClassifier.predict_proba); host default ----------------
    def sparse_code(self, W, X, P=None, max_iter=1000, n_jobs=None):
        """Non-negative LARS-lasso code of the rows of X over the rows of W, scikit-learn's
        ``SparseCoder(normalize(W), "lasso_lars", positive_code=True, transform_alpha=0)`` on
        ``normalize(X)`` (BaseSom.py:241-268).  P (M x C) given: returns the class probabilities
        ``code @ P`` normalised per row (SomClassifier.py:178-220) instead of the code."""
        from sklearn.decomposition import SparseCoder
        from sklearn.preprocessing import normalize

        coder = SparseCoder(dictionary=normalize(np.asarray(W)), n_jobs=n_jobs, positive_code=True,
                            transform_alpha=0, transform_algorithm="lasso_lars",
                            transform_max_iter=max_iter)
        code = coder.transform(normalize(X))
        if P is None:
            return code
        raw = code @ P
        return raw / raw.sum(axis=1)[np.newaxis].T

    # -- topographic function (BaseSom.topographic_function / phi); host default ------------------------
    def topographic_function(self, W, X, coords, want_distances=False):
        """The two integer histograms that phi(k) of BaseSom.py:955-998 is made of, for the graph with an
        edge {a, b} for every row (a, b) of the 2-BMU pairs of X under W:
            hist_pos[c] (n_pos = max Chebyshev extent of coords + 1): ordered edges by the Chebyshev
                        distance c of their lattice coordinates
            hist_neg[t] (M + 1): ordered lattice 4-neighbour pairs by hop distance t; [M]: no path
        -> (hist_pos, hist_neg, D or None), int64; D (M x M int32, -1 = unreachable) with want_distances.
        Unweighted shortest paths give the integers of the reference's Floyd-Warshall without its O(M^3)."""
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import shortest_path

        xy = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
        M = xy.shape[0]
        _, idx = self.bmu(W, 2, X=X)
        a, b = idx[:, 0], idx[:, 1]
        keep = a != b
        A = csr_matrix((np.ones(2 * int(keep.sum())), (np.r_[a[keep], b[keep]], np.r_[b[keep], a[keep]])),
                       shape=(M, M))
        A.sum_duplicates()
        D = shortest_path(A, unweighted=True, directed=False)
        n_pos = int((xy.max(axis=0) - xy.min(axis=0)).max()) + 1
        r, c = A.nonzero()
        hist_pos = np.bincount(np.abs(xy[r] - xy[c]).max(axis=1), minlength=n_pos).astype(np.int64)
        where = {tuple(p): i for i, p in enumerate(xy.tolist())}
        i_nb, j_nb = [], []
        for i, (x, y) in enumerate(xy.tolist()):
            for p in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                j = where.get(p)
                if j is not None:
                    i_nb.append(i)
                    j_nb.append(j)
        t = D[np.asarray(i_nb, dtype=np.int64), np.asarray(j_nb, dtype=np.int64)]
        t = np.where(np.isinf(t), M, t).astype(np.int64)
        hist_neg = np.bincount(t, minlength=M + 1).astype(np.int64)
        Dout = np.where(np.isinf(D), -1, D).astype(np.int32) if want_distances else None
        return hist_pos, hist_neg, Dout

    def release(self):
        pass

    def __deepcopy__(self, memo):
        # sklearn.clone deep-copies constructor parameters; device handles are not copyable,
        # a fresh backend with the same configuration is what a cloned estimator needs
        return self.__class__(*getattr(self, "_init_args", ()))


def is_sparse(X) -> bool:
    """Whether X is a scipy sparse matrix / array (scipy is only imported when it already is)."""
    import sys

    sp = sys.modules.get("scipy.sparse")
    return sp is not None and sp.issparse(X)


def is_device_array(X) -> bool:
    """Whether X is an array that lives in GPU memory: anything with ``data_ptr()``, ``shape``, ``stride()``,
    ``dtype`` and a ``device`` whose ``type`` is ``"cuda"`` -- a torch tensor on a GPU (ROCm builds of PyTorch
    call the device "cuda" too).  A CPU tensor is not one: it goes through ``check_array`` like any host array."""
    if not all(hasattr(X, a) for a in ("data_ptr", "shape", "stride", "dtype", "device")):
        return False
    return getattr(X.device, "type", None) == "cuda"


def array_namespace(X):
    """The module whose functions make arrays like X (``empty``, ``asarray``, ``isfinite``, ...): what X names
    through the array API's ``__array_namespace__``, else the package its class comes from (``torch``)."""
    if hasattr(X, "__array_namespace__"):
        return X.__array_namespace__()
    import importlib

    return importlib.import_module(type(X).__module__.split(".")[0])


def dtype_name(X) -> str:
    """"float32" for torch.float32, numpy.float32 and the like."""
    return str(X.dtype).split(".")[-1]


def device_empty(like, shape, dtype: str):
    """An uninitialised array of `shape` and dtype `dtype` ("int64", "float64") next to `like`, made by like's
    own namespace."""
    ns = array_namespace(like)
    return ns.empty(tuple(int(v) for v in shape), dtype=getattr(ns, dtype), device=like.device)


def canonical_csr(X):
    """X as canonical CSR for the device: column indices ascending and without duplicates within a row (made
    so on a copy when they are not), float32 kept, anything else but float64 converted to float64 as dense
    input is, `indices` int32, `indptr` int64 -> (csr, indptr, indices, data)."""
    import scipy.sparse as sp

    csr = sp.csr_matrix(X)   # (CSC / COO / ... are converted; a CSR matrix is not copied)
    if csr.dtype not in (np.float32, np.float64):
        csr = csr.astype(np.float64)
    if csr.ndim != 2 or csr.shape[0] < 1:
        raise ValueError("X must be a non-empty 2-D array")
    if not csr.has_canonical_format:
        csr = csr.copy()         # (csr_matrix(X) shares X's arrays: the caller's matrix stays as it is)
        csr.sum_duplicates()     # (sorts the indices first)
    if csr.shape[1] > np.iinfo(np.int32).max:
        raise ValueError("too many features for int32 column indices")
    indptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
    data = np.ascontiguousarray(csr.data)
    return csr, indptr, indices, data


def _x_dtype_code(dt) -> int:
    if isinstance(dt, str) and dt == "bf16":
        return _native.BF16
    if dt == np.float32:
        return _native.F32
    if dt == np.float64:
        return _native.F64
    raise ValueError(f"samples must be float32 or float64, got {dt}")


_DTYPE_CODES = {"float32": _native.F32, "float64": _native.F64, "bfloat16": _native.BF16}   # by dtype_name()
_CODE_DTYPES = {_native.F32: np.dtype(np.float32), _native.F64: np.dtype(np.float64), _native.BF16: "bf16"}


def host_rows(X):
    """X as the host-array calls take it: C-contiguous, float32 / float64 kept, anything else (integer / half
    input) as float64, as check_array would."""
    X = np.ascontiguousarray(X)
    return X if X.dtype in (np.float32, np.float64) else X.astype(np.float64)


def round_f32(x_dtype, W) -> int:
    """float32 samples AND float32 prototypes: the reference's engine returns float32-rounded distances (epoch 0
    of a float32 fit).  Every other mix is full float64.  ``x_dtype``: the rows' dtype or its name."""
    return int(str(x_dtype) == "float32" and W is not RESIDENT and np.asarray(W).dtype == np.float32)


HOST, DEVICE, CSR = "", "_device", "_csr"   # the three forms of a query's rows: the suffix of their entry points


class _QueryRows:
    """The rows X of a query as the C ABI takes them, and the only place that tells the three forms apart: a host
    array (converted by ``host_rows``), an array in HBM (``is_device_array``, taken as it is) or a scipy sparse
    matrix (made canonical CSR).  ``suffix`` selects the entry point, ``N``, ``d`` and ``dtype`` (a name) are what a
    caller checks W against -- both None when X is not 2-D, which no W matches --, ``args()`` is the head of the C
    argument list, ``empty`` / ``full`` / ``ptr`` make and pass outputs next to X, ``before_call`` is what has to
    happen right in front of the call.  ``forms``: what the caller accepts; ``name`` says whose refusal it is.

    Device rows are validated (``_device_rows``) and sparse rows made canonical when the object is made, or with
    ``defer`` when they are first needed -- ``empty`` on device rows, ``args`` -- for the callers that check W and
    their own arguments against X's shape first, and return without a call, before ``canonical_csr`` would refuse
    them, when X has no rows."""

    def __init__(self, backend, X, forms, name, defer):
        self.suffix = CSR if is_sparse(X) else DEVICE if is_device_array(X) else HOST
        if self.suffix == CSR and CSR not in forms:
            raise TypeError(f"the {name} calls take dense rows")
        if self.suffix == DEVICE and DEVICE not in forms:
            raise TypeError(f"the {name} calls take host rows")
        self._backend, self._args = backend, None
        self.X = host_rows(X) if self.suffix == HOST else X
        self.N, self.d = (int(v) for v in self.X.shape) if len(self.X.shape) == 2 else (None, None)
        self.dtype = dtype_name(self.X)
        if not defer:
            self.args()

    def args(self, null_when_empty=False):
        """host: (ptr, code, N, d); device: (ptr, code, N, d, ldx); CSR: (indptr, indices, data, code, N, d, nnz)"""
        if self._args is None:
            X = self.X
            if self.suffix == DEVICE:
                self._args = (ctypes.c_void_p(X.data_ptr()),) + self._backend._device_rows(X)
            elif self.suffix == CSR:
                csr, indptr, indices, data = canonical_csr(X)
                self._keep = (indptr, indices, data)
                self._args = (indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, _x_dtype_code(data.dtype),
                              csr.shape[0], csr.shape[1], data.size)
            else:
                self._args = (X.ctypes.data, _x_dtype_code(X.dtype), self.N, self.d)
        return (None,) + self._args[1:] if null_when_empty and not self.N else self._args

    def empty(self, shape, dtype: str):
        if self.suffix != DEVICE:
            return np.empty(shape, dtype=dtype)
        self.args()   # (rows that _device_rows refuses get no output)
        return device_empty(self.X, shape, dtype)

    def full(self, shape, value, dtype: str):
        if self.suffix != DEVICE:
            return np.full(shape, value, dtype=dtype)
        ns = array_namespace(self.X)
        return ns.full(shape, value, dtype=getattr(ns, dtype), device=self.X.device)

    def ptr(self, out):
        return ctypes.c_void_p(out.data_ptr()) if self.suffix == DEVICE else out.ctypes.data

    def ld(self, n):
        """The row stride that follows a matrix output of n columns: only the device calls take one."""
        return (n,) if self.suffix == DEVICE else ()

    def before_call(self):
        if self.suffix == DEVICE:
            self._backend._producer_done(self.X)


class _Resident:
    """Stands for "the prototypes resident in HBM" wherever a weight matrix is expected."""

    def __repr__(self):
        return "RESIDENT"


RESIDENT = _Resident()


class _DeviceArray:
    """A float64 vector in HBM as an object ``torch.as_tensor`` can alias (no copy)."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f8",
                                         "data": (int(ptr), False), "version": 3, "strides": None}


_RCCL_COMMS = {}   # (device index, world, rank) -> ncclComm_t made by dbgsom_rccl_comm_init (process lifetime;
                    # a process group rebuilt with another size or rank gets a communicator of its own)


class HipBackend(HotPathBackend):
    """MI355X backend: one ``dbgsom_ctx`` (one GPU) per instance / process."""

    name = "hip"

    # the filtered search pays off once the all-pairs float64 work is large (mirrors csrc/search_policy.h;
    # tests/test_search_policy_cpu.py checks every mirrored value against the header)
    FILTER_MIN_PROTOTYPES = 129
    FILTER_MAX_FEATURES = 43690
    FILTER_MAX_MEAN_CANDIDATES = 320
    FILTER_MIN_QUERY_ROWS = 32768
    # the PRIOR of the engine's search policy (search_policy.h: SearchPolicy::adapt_arms): what an arm that has never
    # been timed is priced at; arms that have run clean are compared by the engine's clock (arm_ms()).  Mirrored here
    # only for the test of the prior on small inputs, where every epoch copies results to the host and nothing is timed.
    SWEEP_COST = {1: 0.35, 2: 1.0, 3: 1.96}
    LIST_COST = 12.5
    PRUNE_PASS_COST = 60.0

    def __init__(self, device: Optional[int] = None, algorithm: str = "auto", _ctx=None):
        """algorithm (all give IDENTICAL results):
          "exact"          all-pairs float64 MFMA search;
          "filtered"       stateless: coarse int8-MFMA pre-pass -> int8 candidate sweep -> exact
                           float64 search on the candidates; nothing from earlier epochs is used;
          "filtered_hint"  the same, but the previous epoch's winners replace the pre-pass when
                           they are available (training: they almost always still win);
          "auto"           "filtered_hint" with a back-off to "exact" while the candidate lists are
                           long (maps of near-duplicate prototypes).
        The filtered forms apply to 129 <= M <= 16000 prototypes and rows of up to 43690 features
        (float32, float64 or bfloat16-resident samples); otherwise the exact kernel runs."""
        self._lib = _native.load()  # raises when the extension is not built
        if algorithm not in _native.ALGORITHMS:
            raise ValueError("algorithm must be 'auto', 'exact', 'filtered' or 'filtered_hint'")
        self._init_args = (device, algorithm)
        n_dev = _native.device_count()
        if n_dev < 1:
            raise RuntimeError(
                "dbgsom_amd.HipBackend needs a visible AMD GPU (MI355X / gfx950); found "
                f"hipGetDeviceCount()={n_dev}. There is no CPU fallback in the product path.")
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) % n_dev
        self.device_index = int(device)
        self._ctx = ctypes.c_void_p()
        if _ctx is not None:
            self._ctx = _ctx            # adopted (a Voronoi subset made on the device)
        else:
            _native.call("dbgsom_ctx_create", self.device_index, ctypes.byref(self._ctx))
        self._set("algorithm", _native.ALGORITHMS[algorithm])
        self._loaded = _ctx is not None
        self._borrowed = None       # keeps an adopted device array alive
        self._hop_key = None
        self._cb = None
        self._cb_error = None
        self._last_M = 0
        self._part_M = 0            # (units of the last partition; none yet: dbgsom_ctx_read_partition refuses)
        self._x_traffic = {k: 0 for k in self._X_TRAFFIC}   # of contexts released since, and of fetch / put
        self.filter_log = []        # (epoch kind, mean candidates, digit planes) of the last epochs
        self.phase_log = None       # bench hook: a list collects the per-epoch phase times (ms)
        if _ctx is not None:
            self._N, self._d = self._get("n_samples"), self._get("features")
            self._x_np_dtype = _CODE_DTYPES[self._get("storage")]
        self._install_collective()

    # -- plumbing -------------------------------------------------------------------------------
    def _set(self, name, value):
        _native.call("dbgsom_ctx_set_option", self._ctx, name.encode(), int(value))

    def _get(self, name) -> int:
        v = ctypes.c_int64(0)
        _native.call("dbgsom_ctx_get_option", self._ctx, name.encode(), ctypes.byref(v))
        return int(v.value)

    def _call(self, fn, *args):
        self._cb_error = None
        try:
            _native.call(fn, *args)
        except _native.DbgsomNativeError:
            if self._cb_error is not None:
                raise self._cb_error
            raise

    algorithm = property(lambda self: {v: k for k, v in _native.ALGORITHMS.items()}[self._get("algorithm")],
                         lambda self, a: self._set("algorithm", _native.ALGORITHMS[a]))
    # digit planes of the candidate sweep: 0 = adaptive, 1 = one int8 digit product (coarsest
    # bound), 2 = three, 3 = six (tightest); results do not depend on it
    sweep_planes = property(lambda self: self._get("sweep_planes"),
                            lambda self, v: self._set("sweep_planes", v))
    # the stateless seed pre-pass looks at every seed_stride-th prototype (0 = library default)
    seed_stride = property(lambda self: self._get("seed_stride"),
                           lambda self, v: self._set("seed_stride", v))
    # per-sample refinement in front of the exact stage of the filtered search (filter.hip 2d)
    # 0 / False = off, 1 / True = on, 2 = by measurement (the default): the engine times the exact stage of
    # the first epochs of a map size with and without it and keeps the faster form
    refine = property(lambda self: self._get("refine"), lambda self, v: self._set("refine", int(v)))
    refined = property(lambda self: bool(self._get("refined")))   # what the last filtered search ran
    # neighbourhood smoothing sharded over the ranks (reduce-scatter of column blocks of the sums, all-gather of
    # the new prototypes): 0 never, 1 whenever the collective can, 2 (default) on large maps
    shard_smooth = property(lambda self: self._get("shard_smooth"), lambda self, v: self._set("shard_smooth", int(v)))
    shard_epochs = property(lambda self: self._get("shard_epochs"))
    # CSR input of fewer features than this is expanded into dense rows on the device (0: never); results do
    # not depend on it.  resident_csr: whether the loaded samples are a CSR resident
    csr_densify_below = property(lambda self: self._get("csr_densify_below"),
                                 lambda self, v: self._set("csr_densify_below", int(v)))
    resident_csr = property(lambda self: bool(self._get("resident_csr")))
    planes_cached = property(lambda self: bool(self._get("planes_cached")))
    # the stateless pruning search of the resident samples takes its seeds from anchor buckets built once per load
    # (filter.hip 2e) instead of a seed pre-pass per epoch: 1 (default) / 0; results do not depend on it.
    # anchor_builds: how often they were built; anchor_state: 0 none, 1 in use, 2 dropped (longer lists than the
    # pre-pass's on this sample set).  A caller's seed_stride keeps the policy on the cheap seeds (no full pre-pass).
    anchor_seeds = property(lambda self: self._get("anchor_seeds"), lambda self, v: self._set("anchor_seeds", int(v)))
    anchor_builds = property(lambda self: self._get("anchor_builds"))
    anchor_searches = property(lambda self: self._get("anchor_searches"))   # searches seeded from them so far
    lean_searches = property(lambda self: self._get("lean_searches"))   # epochs among them in the lean form
    anchor_state = property(lambda self: self._get("anchor_state"))
    padded_features = property(lambda self: self._get("padded_features"))

    @property
    def n_samples(self):
        return self._get("n_samples")

    def _require_loaded(self):
        if not self._loaded:
            raise RuntimeError("HipBackend: call load(X) first")

    # -- the one collective ---------------------------------------------------------------------
    def _install_collective(self):
        """Plug torch.distributed's all-reduce into the context when a process group is up (or
        DBGSOM_FORCE_COLLECTIVE=1 asks for the rehearsal of that path with one rank)."""
        rank, world = dist_info()
        force = os.environ.get("DBGSOM_FORCE_COLLECTIVE") == "1" and _group_is_up()
        if world == 1 and not force:
            _native.call("dbgsom_ctx_set_collectives", self._ctx, None, None, 0, 1)
            self._cb = None
            return
        import torch
        import torch.distributed as td

        dev = torch.device("cuda", self.device_index)
        on_device = td.get_backend() == "nccl"
        if on_device and os.environ.get("DBGSOM_COLLECTIVE", "rccl") != "callback":
            # RCCL driven by the library itself (dbgsom_ctx_set_rccl): no callback, no interpreter in the
            # epoch.  One communicator per process and device, made once (torch.distributed only carries
            # rank 0's 128-byte id to the other ranks) and shared by every context of this process.
            key = (self.device_index, world, rank)
            comm = _RCCL_COMMS.get(key, "untried")
            if comm == "untried":
                # (every rank goes through every step and the ranks then agree on the outcome: a communicator
                #  that came up on some ranks only must not be used by any)
                uid, err = ctypes.create_string_buffer(128), None
                if rank == 0:
                    try:
                        _native.call("dbgsom_rccl_unique_id", uid)
                    except Exception as e:  # noqa: BLE001
                        err = e
                box = [uid.raw if err is None else None]
                td.broadcast_object_list(box, src=0)
                comm = ctypes.c_void_p()
                if box[0] is not None:
                    try:
                        uid = ctypes.create_string_buffer(box[0], 128)
                        self._get("n_samples")   # (a context call: this thread is on the context's device)
                        _native.call("dbgsom_rccl_comm_init", uid, world, rank, ctypes.byref(comm))
                    except Exception as e:  # noqa: BLE001
                        err, comm = e, ctypes.c_void_p()
                else:
                    err = err or RuntimeError("rank 0 could not make an RCCL id")
                ok = torch.tensor([1 if (err is None and comm.value) else 0], device=dev, dtype=torch.int32)
                td.all_reduce(ok, op=td.ReduceOp.MIN)
                if int(ok.item()) == 1:
                    _RCCL_COMMS[key] = comm
                else:
                    # the library could not drive RCCL itself in this process (its librccl is not the one of the
                    # HIP runtime in use, say): the same collectives through torch.distributed's communicator
                    import warnings
                    warnings.warn(f"dbgsom_amd: RCCL inside the library is unavailable ({err}); "
                                  "collectives go through torch.distributed")
                    _RCCL_COMMS[key] = comm = None
            if comm is not None:
                _native.call("dbgsom_ctx_set_rccl", self._ctx, comm)
                self._cb = None
                return
        cache = {}   # the context reuses its stream and (until the map grows) its buffers

        def collective(_user, op, ptr, count, stream):
            """dbgsom_collective_fn: all-reduce of `count` values, or -- for the smoothing sharded over the
            ranks -- reduce-scatter / all-gather in place over `world` blocks of `count` values."""
            try:
                ext = cache.get(("stream", stream))
                if ext is None:
                    ext = cache[("stream", stream)] = torch.cuda.ExternalStream(stream, device=dev)
                total = count if op == _native.COLL_ALLREDUCE else count * world
                with torch.cuda.stream(ext):
                    t = cache.get((ptr, total))
                    if t is None:
                        if len(cache) > 16:
                            cache.clear()
                            cache[("stream", stream)] = ext
                        t = cache[(ptr, total)] = torch.as_tensor(_DeviceArray(ptr, total), device=dev)
                    mine = t[rank * count:(rank + 1) * count] if op != _native.COLL_ALLREDUCE else None
                    if on_device:   # RCCL through torch.distributed, ordered on the context's stream
                        if op == _native.COLL_ALLREDUCE:
                            td.all_reduce(t, op=td.ReduceOp.SUM)
                        elif op == _native.COLL_REDUCE_SCATTER:
                            td.reduce_scatter_tensor(mine, t, op=td.ReduceOp.SUM)
                        else:
                            td.all_gather_into_tensor(t, mine.clone())
                    else:  # gloo and friends: through the host (tests: several ranks on one GPU)
                        h = t.cpu()
                        if op == _native.COLL_ALLREDUCE:
                            td.all_reduce(h, op=td.ReduceOp.SUM)
                            t.copy_(h)
                        elif op == _native.COLL_REDUCE_SCATTER:
                            # (gloo has no reduce-scatter: a reduce per block to its owner -- every block is
                            #  summed in one order, whoever owns it)
                            for r in range(world):
                                blk = h[r * count:(r + 1) * count]
                                td.reduce(blk, dst=r, op=td.ReduceOp.SUM)
                            mine.copy_(h[rank * count:(rank + 1) * count])
                        else:
                            parts = [torch.empty(count, dtype=h.dtype) for _ in range(world)]
                            td.all_gather(parts, h[rank * count:(rank + 1) * count].contiguous())
                            t.copy_(torch.cat(parts))
                        ext.synchronize()
                return 0
            except BaseException as e:  # nothing may propagate through the C frames
                self._cb_error = e
                return 1

        self._cb = _native.COLLECTIVE_FN(collective)
        _native.call("dbgsom_ctx_set_collectives", self._ctx, self._cb, None, rank, world)

    # -- a8: residency --------------------------------------------------------------------------
    def load(self, X, storage=None, incomplete=False):
        """Upload the samples once.  `storage="bf16"` keeps them in HBM as bfloat16 (rounded to
        nearest even on the device; all arithmetic stays float64 on the exactly widened values --
        an extension, the reference has no bf16).  A scipy sparse matrix is made canonical CSR and loaded as such
        (``dbgsom_ctx_load_csr``): below ``csr_densify_below`` features it is expanded on the device into the
        dense resident form, at and above it the CSR kernels run -- the same results either way.
        ``incomplete=True``: NaN in X (dense float32 / float64, native storage) marks a missing entry.  The rows'
        observed-entry counts and, for float32 rows, a float64 copy (N x d x 8 bytes of HBM) are made once;
        ``bmu(W, k)`` is then the masked search, ``epoch_masked`` the epoch, and the ordinary epoch / update /
        partition calls raise."""
        if incomplete and (is_sparse(X) or storage not in (None, "native")):
            raise ValueError("incomplete=True takes dense rows in their own dtype")
        if is_sparse(X):
            if storage not in (None, "native"):
                raise ValueError("sparse input cannot be stored as bf16")
            csr, indptr, indices, data = canonical_csr(X)
            self._call("dbgsom_ctx_load_csr", self._ctx, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data,
                       _x_dtype_code(data.dtype), csr.shape[0], csr.shape[1], data.size)
            self._after_load(csr.shape, data.dtype)
            self._borrowed = None
            return self
        X = host_rows(X)
        code = _x_dtype_code(X.dtype)
        if X.ndim != 2 or X.shape[0] < 1:
            raise ValueError("X must be a non-empty 2-D array")
        if storage == "bf16":
            if X.dtype != np.float32:
                X = X.astype(np.float32)
                code = _native.F32
            st = _native.BF16
        elif storage in (None, "native"):
            st = code
        else:
            raise ValueError("storage must be None or 'bf16'")
        self._call("dbgsom_ctx_load", self._ctx, X.ctypes.data, code, X.shape[0], X.shape[1], st)
        self._after_load(X.shape, "bf16" if st == _native.BF16 else X.dtype)
        self._borrowed = None
        if incomplete:
            self._set("incomplete", 1)
            self._incomplete = True
        return self

    @staticmethod
    def _producer_done(X_dev):
        """Wait for the torch stream X_dev was produced on (its producer may still be running)."""
        if type(X_dev).__module__.split(".")[0] == "torch":
            import torch

            torch.cuda.current_stream(X_dev.device).synchronize()

    def _device_rows(self, X_dev, dtypes=("float32", "float64")):
        """-> (dtype code, N, d, row stride) of rows in HBM a *_device entry point can take as they are."""
        code = _DTYPE_CODES.get(dtype_name(X_dev))
        if code is None or dtype_name(X_dev) not in dtypes or len(X_dev.shape) != 2:
            raise ValueError("device rows must be a 2-D array of " + " / ".join(dtypes))
        N, d = int(X_dev.shape[0]), int(X_dev.shape[1])
        if X_dev.stride(1) != 1 or (N > 1 and X_dev.stride(0) < d):
            raise ValueError("device rows need unit column stride and a row stride of at least their length")
        index = getattr(X_dev.device, "index", None)
        if index is not None and index != self.device_index:
            raise ValueError(f"the rows live on GPU {index}, this backend runs on GPU {self.device_index}")
        return code, N, d, int(X_dev.stride(0)) if N > 1 else d

    def load_device(self, X_dev):
        """Adopt samples that already live in HBM: anything with `data_ptr()`, `shape`, `stride()`
        and a float32 / float64 / bfloat16 dtype (a torch tensor; bench: generated on the device).
        The caller's writes must have completed; the array is borrowed when its rows are a
        multiple of 16 features, copied (padded) otherwise."""
        code = _DTYPE_CODES.get(dtype_name(X_dev))
        if code is None or len(X_dev.shape) != 2 or X_dev.stride(1) != 1:
            raise ValueError("X_dev must be a 2-D float32/float64/bfloat16 array with unit column stride")
        N, d = int(X_dev.shape[0]), int(X_dev.shape[1])
        index = getattr(getattr(X_dev, "device", None), "index", None)
        if index is not None and index != self.device_index:
            raise ValueError(f"the rows live on GPU {index}, this backend runs on GPU {self.device_index}")
        self._producer_done(X_dev)
        self._call("dbgsom_ctx_load_device", self._ctx, ctypes.c_void_p(X_dev.data_ptr()), code, N, d,
                   int(X_dev.stride(0)))
        self._after_load((N, d), _CODE_DTYPES[code])
        self._borrowed = X_dev
        return self

    def _after_load(self, shape, np_dtype):
        self._N, self._d = int(shape[0]), int(shape[1])
        self._x_np_dtype = np_dtype
        self._loaded = True
        self.resident_serial += 1
        self._hop_key = None
        self._last_M = 0
        self._part_M = 0            # (units of the last partition; none yet: dbgsom_ctx_read_partition refuses)
        self._y = None
        self._sw = None          # (a load detaches the weights of the rows that were resident)
        self._weighted = False
        self._incomplete = False
        self._metric = "euclidean"
        self._targets = None     # (and the targets)
        self._targets_attached = False

    def read_samples(self, rows):
        """Rows of the resident samples as float64 (exactly widened)."""
        self._require_loaded()
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((rows.size, self._d))
        self._call("dbgsom_ctx_read_samples", self._ctx, rows.ctypes.data, rows.size, out.ctypes.data)
        return out

    # -- prototypes -----------------------------------------------------------------------------
    def _w_arg(self, W, d=None):
        """-> (keep-alive array, pointer or None, M, round_f32) for a weight argument."""
        if W is RESIDENT:
            M = self._get("prototypes")
            if M < 1:
                raise RuntimeError("no prototypes resident in HBM yet")
            return None, None, M, 0
        rf = round_f32(self._x_np_dtype, W) if d is None else 0
        W64 = np.ascontiguousarray(W, dtype=np.float64)
        if W64.ndim != 2 or W64.shape[1] != (self._d if d is None else d):
            raise ValueError("prototype / sample feature mismatch")
        return W64, W64.ctypes.data, W64.shape[0], rf

    def set_weights(self, W):
        self._require_loaded()
        keep, p, M, _ = self._w_arg(W)
        self._call("dbgsom_ctx_set_weights", self._ctx, p, M)
        return RESIDENT

    def get_weights(self, which=0):
        """which=0: the resident prototypes; 1: the other buffer (after an epoch: its input)."""
        M = self._get("prototypes") if which == 0 else self._last_M
        out = np.empty((M, self._d))
        self._call("dbgsom_ctx_get_weights", self._ctx, int(which), out.ctypes.data, M)
        return out

    def read_weight_rows(self, rows, which=0):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((rows.size, self._d))
        self._call("dbgsom_ctx_read_weight_rows", self._ctx, int(which), rows.ctypes.data, rows.size,
                   out.ctypes.data)
        return out

    def write_weight_rows(self, row0, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, self._d)
        self._call("dbgsom_ctx_write_weight_rows", self._ctx, int(row0), rows.shape[0], rows.ctypes.data)

    # -- a1 -------------------------------------------------------------------------------------
    def bmu(self, W, k=1, X=None):
        """-> (distances, winners) like BaseSom._get_winning_neurons: shape (N,) for k=1,
        (N, k) otherwise."""
        if X is None:
            self._require_loaded()
            if self._incomplete and W is RESIDENT:
                raise ValueError("no prototypes stay resident between masked epochs")
            if self._manhattan and W is RESIDENT:
                raise ValueError("no prototypes stay resident between Manhattan epochs")
            if self._cosine and W is RESIDENT:
                raise ValueError("no prototypes stay resident between cosine epochs")
            keep, p, M, rf = self._w_arg(W, d=self._d if self._incomplete or self._other_metric else None)
            N = self._N
            idx = np.empty((N, k), dtype=np.int64)
            dist = np.empty((N, k), dtype=np.float64)
            if self._manhattan:    # metric="manhattan": the L1 search of the resident rows
                self._call("dbgsom_ctx_bmu_manhattan", self._ctx, p, M, int(k), idx.ctypes.data, dist.ctypes.data)
            elif self._cosine:     # metric="cosine": the cosine search of the resident rows
                self._call("dbgsom_ctx_bmu_cosine", self._ctx, p, M, int(k), idx.ctypes.data, dist.ctypes.data)
            elif self._incomplete:   # rows with missing entries: the search over the observed entries of every row
                self._call("dbgsom_ctx_bmu_masked", self._ctx, p, M, int(k), idx.ctypes.data, dist.ctypes.data)
            else:
                self._call("dbgsom_ctx_bmu", self._ctx, p, M, int(k), rf, idx.ctypes.data, dist.ctypes.data)
        else:
            return self._bmu_query("euclidean", W, k, X)
        return self._bmu_shapes(dist, idx, k)

    @staticmethod
    def _bmu_shapes(dist, idx, k):
        """(N, k) results in ``bmu``'s shapes: (N,) for k = 1"""
        return (dist.reshape(-1), idx.reshape(-1)) if k == 1 else (dist, idx)

    # -- queries on other rows: one marshaller for host arrays, arrays in HBM and CSR ------------------------
    _DENSE = (HOST, DEVICE)
    _QUERY_ROWS = {"euclidean": ((HOST, DEVICE, CSR), None), "manhattan": (_DENSE, "Manhattan"),
                   "cosine": (_DENSE, "cosine"), "masked": ((HOST,), "masked"), "sparse coding": (_DENSE, "sparse coding"),
                   "topographic function": (_DENSE, "topographic function"),
                   "row_neighbors": (_DENSE, "row_neighbors")}   # what takes which rows

    def _query_rows(self, X, kind="euclidean", defer=False):
        return _QueryRows(self, X, *self._QUERY_ROWS[kind], defer)

    def _query(self, op, metric, rows, *rest, null_when_empty=False):
        """The one call of a query: dbgsom_ctx_<op>[_<metric>][_device | _csr](ctx, the rows, rest...); with
        ``null_when_empty`` rows that are none go as a null pointer."""
        infix = "" if metric == "euclidean" else "_" + metric
        rows.before_call()
        self._call(f"dbgsom_ctx_{op}{infix}{rows.suffix}", self._ctx, *rows.args(null_when_empty), *rest)

    @staticmethod
    def _w64(W, d):
        """-> (W as contiguous float64, M), checked against rows of d features"""
        W64 = np.ascontiguousarray(W, dtype=np.float64)
        if W64.ndim != 2 or W64.shape[1] != d:
            raise ValueError("prototype / sample feature mismatch")
        return W64, W64.shape[0]

    def _bmu_query(self, metric, W, k, X, want_filled=False):
        """``bmu(W, k, X=X)`` under ``metric`` ("euclidean", "manhattan", "cosine", or "masked": over the observed
        entries) on the device: host rows go up in chunks (``masked_chunk_rows`` rows for the other metrics), CSR rows
        are searched as they are (dbgsom_ctx_bmu_query_csr); for rows in HBM the searches run on X's own bytes and
        distances and winners are arrays on X's device that the search writes itself.  ``want_filled`` ("masked"):
        the filled rows are a third result."""
        euclidean = metric == "euclidean"
        rows = self._query_rows(X, metric)
        W64, M = self._w64(W, rows.d)
        k = int(k)
        filled = np.empty_like(rows.X) if want_filled else None
        idx, dist = rows.empty((rows.N, k), "int64"), rows.empty((rows.N, k), "float64")
        rf = (round_f32(rows.dtype, W),) if euclidean else ()     # (only the Euclidean search rounds to float32)
        extra = (None if filled is None else filled.ctypes.data,) if metric == "masked" else ()
        # (the other metrics take rows that are none as a null pointer from the host and launch nothing for them in HBM)
        if euclidean or rows.N or rows.suffix == HOST:
            self._query("bmu_query", metric, rows, W64.ctypes.data, M, k, *rf, rows.ptr(idx), rows.ptr(dist), *extra,
                        null_when_empty=not euclidean)
        dist, idx = self._bmu_shapes(dist, idx, k)
        return (dist, idx, filled) if want_filled else (dist, idx)

    def resident_winners(self, W):
        """``bmu(W, 1)[1]`` of the resident samples without the distances' trip to the host."""
        self._require_loaded()
        if self._incomplete or self._other_metric:
            return self.bmu(W, 1)[1]
        keep, p, M, rf = self._w_arg(W)
        idx = np.empty(self._N, dtype=np.int64)
        self._call("dbgsom_ctx_bmu", self._ctx, p, M, 1, rf, idx.ctypes.data, None)
        return idx

    # -- per-row results between HBM and the host ------------------------------------------------------
    def fetch(self, t) -> np.ndarray:
        """A per-row result that lives in HBM as a NumPy array (counted as sample traffic)."""
        out = t.cpu().numpy()
        self._x_traffic["x_download_bytes"] += out.nbytes
        return out

    def put(self, a, like):
        """A per-row result on the host as an array next to `like` (counted as sample traffic)."""
        a = np.ascontiguousarray(a)
        self._x_traffic["x_upload_bytes"] += a.nbytes
        self._x_traffic["x_upload_calls"] += 1
        return array_namespace(like).asarray(a, device=like.device)

    # -- rows with missing entries ------------------------------------------------------------------
    masked_chunk_rows = property(lambda self: self._get("masked_chunk_rows"),
                                 lambda self, v: self._set("masked_chunk_rows", v))

    def bmu_masked(self, W, k, X, want_filled=False):
        """The search over the observed entries of every row on the device (csrc/masked.hip), in chunks of
        ``masked_chunk_rows`` rows; with ``want_filled`` each chunk is filled there after its search."""
        return self._bmu_query("masked", W, k, X, want_filled)

    # -- the distance matrix of a query ----------------------------------------------------------------
    # rows per chunk of the host-array calls (0, the default: as many as keep a chunk's staged result at 256 MiB)
    distances_chunk_rows = property(lambda self: self._get("distances_chunk_rows"),
                                    lambda self, v: self._set("distances_chunk_rows", v))

    def distances(self, W, X):
        """Every distance the all-pairs search of ``bmu(W, k, X=X)`` computes (csrc/distances.hip), stored instead of
        reduced.  Host rows go up and the matrix comes down in chunks of ``distances_chunk_rows`` rows; CSR rows are
        expanded on the device chunk by chunk; for rows in HBM the result is a float64 array on their device that
        the kernel writes itself (dbgsom_ctx_distances_query_device)."""
        return self._distances("euclidean", W, X)

    def _distances(self, metric, W, X):
        """``distances`` under ``metric``.  The Euclidean call checks W against X's shape before it looks at the rows
        (and so do ``kneighbors`` and the calls below it), the other metrics after."""
        rows = self._query_rows(X, metric, defer=metric == "euclidean")
        W64, M = self._w64(W, rows.d)
        out = rows.empty((rows.N, M), "float64")
        if rows.N:
            self._query("distances_query", metric, rows, W64.ctypes.data, M, rows.ptr(out), *rows.ld(M))
        return out

    def distances_masked(self, W, X):
        """The distances over the observed entries of every row on the device (csrc/distances.hip), in chunks of
        ``distances_chunk_rows`` rows."""
        return self._distances("masked", W, X)

    # -- the k nearest prototypes of a query -----------------------------------------------------------
    # rows per slab of squared distances (0, the default: as many, in multiples of 128, as keep the slab at 64 MiB)
    kneighbors_slab_rows = property(lambda self: self._get("kneighbors_slab_rows"),
                                    lambda self, v: self._set("kneighbors_slab_rows", v))

    @staticmethod
    def _check_neighbors(k, M):
        if not 1 <= k <= M:
            raise ValueError(f"need 1 <= k <= {M} prototypes, got k = {k}")
        if k > _native.MAX_NEIGHBORS:
            raise ValueError(f"k = {k} is above DBGSOM_MAX_NEIGHBORS = {_native.MAX_NEIGHBORS}")

    def kneighbors(self, W, k, X):
        """The k nearest prototypes of every row (csrc/kneighbors.hip): the squared distances of a slab of
        ``kneighbors_slab_rows`` rows stay on the device, the selection kernel reads them back from cache, and only
        (rows, k) distances and indices are the result.  Host rows go up in chunks of ``distances_chunk_rows``
        rows; CSR rows are expanded on the device chunk by chunk; for rows in HBM both results are arrays on their
        device that the kernel writes itself (dbgsom_ctx_kneighbors_query_device)."""
        return self._kneighbors("euclidean", W, k, X)

    def _kneighbors(self, metric, W, k, X):
        """``kneighbors`` under ``metric``: the selection kernel reads a slab of that metric's distances back and
        stores what it selected on."""
        rows = self._query_rows(X, metric, defer=metric == "euclidean")
        W64, M = self._w64(W, rows.d)
        k = int(k)
        self._check_neighbors(k, M)
        dist, idx = rows.empty((rows.N, k), "float64"), rows.empty((rows.N, k), "int64")
        if rows.N:
            self._query("kneighbors_query", metric, rows, W64.ctypes.data, M, k, rows.ptr(idx), rows.ptr(dist))
        return dist, idx

    def kneighbors_masked(self, W, k, X):
        """The k nearest prototypes over the observed entries of every row on the device (csrc/kneighbors.hip on the
        masked chain of csrc/distances.hip), in chunks of ``distances_chunk_rows`` rows."""
        return self._kneighbors("masked", W, k, X)

    # -- the distortion measure of a query -------------------------------------------------------------
    def neighborhood_energy(self, W, H, X):
        """The distortion measure of every row (csrc/distortion.hip): the squared distances of a slab of
        ``kneighbors_slab_rows`` rows stay on the device, the energy kernel reads them back from cache against row
        ``bmu`` of H, and only (rows,) values and units are the result.  H goes up once per call.  Host rows go up
        in chunks of ``distances_chunk_rows`` rows; CSR rows are expanded on the device chunk by chunk; for rows in
        HBM both results are arrays on their device that the kernel writes itself
        (dbgsom_ctx_distortion_query_device)."""
        rows = self._query_rows(X, defer=True)
        W64, M = self._w64(W, rows.d)
        H64 = np.ascontiguousarray(H, dtype=np.float64)
        if H64.shape != (M, M):
            raise ValueError(f"H must be ({M}, {M}), one row per prototype, got {H64.shape}")
        e, bmu = rows.empty((rows.N,), "float64"), rows.empty((rows.N,), "int64")
        if rows.N:
            self._query("distortion_query", "euclidean", rows, W64.ctypes.data, M, H64.ctypes.data, rows.ptr(bmu),
                        rows.ptr(e))
        return e, bmu

    # -- the k nearest rows to every prototype ---------------------------------------------------------
    def exemplars(self, W, k, X, own_cell=False):
        """The k nearest rows to every prototype (csrc/exemplars.hip): the squared distances of a slab of
        ``kneighbors_slab_rows`` rows stay on the device, the fold reads them back from cache down their columns into
        a state of (rows of W, k) pairs that lives on the device for the length of the call, and only that state is
        the result.  Host rows go up in chunks of ``distances_chunk_rows`` rows, every chunk folding into the state
        under its first row's number; CSR rows are expanded on the device chunk by chunk; rows of W x k x 16 bytes
        come down, once.  For rows in HBM both results are arrays on their device that the kernel writes itself
        (dbgsom_ctx_exemplars_query_device).  X without rows: all ``(inf, -1)``, no launch."""
        rows = self._query_rows(X, defer=True)
        W64, M = self._w64(W, rows.d)
        k, own = int(k), int(bool(own_cell))
        if not 1 <= k <= _native.MAX_NEIGHBORS:
            raise ValueError(f"need 1 <= k <= DBGSOM_MAX_NEIGHBORS = {_native.MAX_NEIGHBORS}, got k = {k}")
        if rows.N == 0:
            return rows.full((M, k), float("inf"), "float64"), rows.full((M, k), -1, "int64")
        dist, idx = rows.empty((M, k), "float64"), rows.empty((M, k), "int64")
        self._query("exemplars_query", "euclidean", rows, W64.ctypes.data, M, k, own, rows.ptr(idx), rows.ptr(dist))
        return dist, idx

    # -- the rows within a radius of every prototype ---------------------------------------------------
    def range_counts(self, W, thresholds_squared, X):
        """The rows within a radius of every prototype (csrc/density.hip): the squared distances of a slab of
        ``kneighbors_slab_rows`` rows stay on the device, the fold reads them back from cache down their columns and
        adds what passes each threshold into (rows of W, thresholds) int64 counts that live on the device for the
        length of the call, and only those counts are the result.  The thresholds go up once.  Host rows go up in
        chunks of ``distances_chunk_rows`` rows, every chunk folding into the counts; CSR rows are expanded on the
        device chunk by chunk; rows of W x thresholds x 8 bytes come down, once.  For rows in HBM the result is an
        array on their device (dbgsom_ctx_range_counts_query_device).  X without rows: zeros, no launch."""
        rows = self._query_rows(X, defer=True)
        W64, M = self._w64(W, rows.d)
        thr = np.ascontiguousarray(thresholds_squared, dtype=np.float64).reshape(-1)
        if not 1 <= thr.size <= _native.MAX_RADII:
            raise ValueError(f"need 1 .. DBGSOM_MAX_RADII = {_native.MAX_RADII} thresholds, got {thr.size}")
        if rows.N == 0:
            return rows.full((M, thr.size), 0, "int64")
        counts = rows.empty((M, thr.size), "int64")
        self._query("range_counts_query", "euclidean", rows, W64.ctypes.data, M, thr.ctypes.data, thr.size,
                    rows.ptr(counts))
        return counts

    # -- the map as a Gaussian mixture ---------------------------------------------------------------
    def mixture(self, W, log_prior, c, Y, X):
        """The mixture view of every row (csrc/mixture.hip): the squared distances of a slab of
        ``kneighbors_slab_rows`` rows stay on the device, the mixture kernel reads them back from cache against the
        log-priors and Y, and only (rows,) units and log-sums and (rows, n_values) posterior means are the result.
        The log-priors and Y go up once per call.  Host rows go up in chunks of ``distances_chunk_rows`` rows and
        rows x (16 + 8 n_values) bytes come down; CSR rows are expanded on the device chunk by chunk; for rows in HBM
        the results are arrays on their device that the kernel writes itself (dbgsom_ctx_mixture_query_device)."""
        rows = self._query_rows(X, defer=True)
        W64, M = self._w64(W, rows.d)
        a, c, Y64 = _mixture_args(M, log_prior, c, Y)
        V = 0 if Y64 is None else Y64.shape[1]
        unit, lse = rows.empty((rows.N,), "int64"), rows.empty((rows.N,), "float64")
        q = rows.empty((rows.N, V), "float64") if V else None
        if rows.N:
            self._query("mixture_query", "euclidean", rows, W64.ctypes.data, M, a.ctypes.data, c,
                        Y64.ctypes.data if V else None, V, rows.ptr(unit), rows.ptr(lse), rows.ptr(q) if V else None)
        return unit, lse, q

    # -- weighted geodesics and the combined error of a query ------------------------------------------
    @staticmethod
    def _edge_array(edges, M):
        """-> (E, 2) contiguous int32; indices are checked here, so that the device meets none outside [0, M)"""
        E = np.asarray(edges)
        if E.size == 0:
            return np.empty((0, 2), dtype=np.int32)
        if E.ndim != 2 or E.shape[1] != 2 or not np.issubdtype(E.dtype, np.integer):
            raise ValueError(f"edges must be an (E, 2) integer array, got shape {E.shape} of {E.dtype}")
        if E.min() < 0 or E.max() >= M:
            raise ValueError(f"edges hold an index outside [0, {M})")
        return np.ascontiguousarray(E, dtype=np.int32)

    def geodesics(self, W, edges):
        """The M x M geodesics of the lattice (csrc/geodesics.hip): W and the edges go up, the lengths are formed on
        the device, one workgroup per source relaxes its vector in LDS, and the matrix comes down (8 M^2 bytes)."""
        W64 = np.ascontiguousarray(W, dtype=np.float64)
        if W64.ndim != 2:
            raise ValueError("W must be 2-D")
        M, d = W64.shape
        E = self._edge_array(edges, M)
        G = np.empty((M, M), dtype=np.float64)
        self._call("dbgsom_ctx_geodesics", self._ctx, W64.ctypes.data, M, d, E.ctypes.data if len(E) else None, len(E),
                   G.ctypes.data)
        return G

    def combined_error(self, W, edges, X):
        """The combined error of every row (csrc/geodesics.hip): the geodesics of the map are computed once per call
        into a buffer the context owns, the all-pairs k = 2 search runs chunk by chunk (``distances_chunk_rows``) and
        the rows kernel behind it reads a chunk's pairs and distances where the search left them.  Host rows go up
        in chunks; CSR rows are expanded on the device chunk by chunk; for rows in HBM both results are arrays on
        their device that the kernels write themselves (dbgsom_ctx_combined_error_query_device)."""
        rows = self._query_rows(X, defer=True)
        W64, M = self._w64(W, rows.d)
        if M < 2:
            raise ValueError("the combined error needs a map of at least two prototypes")
        E = self._edge_array(edges, M)
        e, units = rows.empty((rows.N,), "float64"), rows.empty((rows.N, 2), "int64")
        if rows.N:
            self._query("combined_error_query", "euclidean", rows, W64.ctypes.data, M, E.ctypes.data if len(E) else None,
                        len(E), rows.ptr(units), rows.ptr(e))
        return e, units

    # -- metric="manhattan" (csrc/manhattan.hip) --------------------------------------------------------
    _manhattan = property(lambda self: self._metric == "manhattan")
    _cosine = property(lambda self: self._metric == "cosine")
    _other_metric = property(lambda self: self._metric != "euclidean")   # the resident search is not the Euclidean one
    _METRIC_NAME = {"manhattan": "Manhattan", "cosine": "cosine", "masked": "masked"}

    def _metric_epoch(self, metric, W, hop, sigma, gamma, layout, want_assignments, n_classes):
        """One epoch under ``metric`` as ONE call of the C ABI: its search of the resident rows (csrc/manhattan.hip;
        the cosine forms of the MFMA kernels) in front of the sums and the smoothing of ``epoch``
        (dbgsom_ctx_epoch_manhattan, dbgsom_ctx_epoch_cosine)."""
        self._require_loaded()
        if W is RESIDENT:
            raise ValueError(f"no prototypes stay resident between {self._METRIC_NAME[metric]} epochs")
        keep, p, M, _ = self._w_arg(W, d=self._d)
        self._topology(hop, M)
        Wn, chg, E, a = np.empty((M, self._d)), np.empty(1), np.empty(M), np.empty(M)
        want = want_assignments or n_classes > 0
        win = np.empty(self._N, dtype=np.int64) if want else None
        dist = np.empty(self._N) if want else None
        self._call(f"dbgsom_ctx_epoch_{metric}", self._ctx, p, M, float(gamma), float(sigma), _native.LAYOUTS[layout],
                   Wn.ctypes.data, chg.ctypes.data, E.ctypes.data, a.ctypes.data,
                   None if win is None else win.ctypes.data, None if dist is None else dist.ctypes.data)
        self._last_M = M
        res = EpochResult(Wn, float(chg[0]), E, a, win if want_assignments else None, dist if want_assignments else None)
        if n_classes > 0:
            res.class_hist = self.class_histogram(win, n_classes, M)
        return res

    def bmu_manhattan(self, W, k, X):
        return self._bmu_query("manhattan", W, k, X)

    def distances_manhattan(self, W, X):
        return self._distances("manhattan", W, X)

    def kneighbors_manhattan(self, W, k, X):
        return self._kneighbors("manhattan", W, k, X)

    def epoch_manhattan(self, W, hop, sigma, gamma, layout="compact", want_assignments=False, n_classes=0):
        return self._metric_epoch("manhattan", W, hop, sigma, gamma, layout, want_assignments, n_classes)

    # -- metric="cosine" (csrc/cosine.hip and the cosine forms of bmu.hip, bmu_dma.hip, distances.hip) ----
    def bmu_cosine(self, W, k, X):
        return self._bmu_query("cosine", W, k, X)

    def distances_cosine(self, W, X):
        return self._distances("cosine", W, X)

    def kneighbors_cosine(self, W, k, X):
        return self._kneighbors("cosine", W, k, X)

    def epoch_cosine(self, W, hop, sigma, gamma, layout="compact", want_assignments=False, n_classes=0):
        return self._metric_epoch("cosine", W, hop, sigma, gamma, layout, want_assignments, n_classes)

    def query_filter_applies(self, N, d, M, k=1):
        """Whether a k-BMU query on N other samples would go through the filtered search."""
        return (k == 1 and self.algorithm != "exact" and N >= self._get("filter_min_query_rows")
                and self.FILTER_MIN_PROTOTYPES <= M <= _native.MAX_PROTOTYPES and d <= self.FILTER_MAX_FEATURES)

    # -- sparse coding --------------------------------------------------------------------------
    sc_chunk_rows = property(lambda self: self._get("sc_chunk_rows"), lambda self, v: self._set("sc_chunk_rows", v))
    sc_cap = property(lambda self: self._get("sc_cap"), lambda self, v: self._set("sc_cap", v))

    def sparse_code(self, W, X, P=None, max_iter=1000, n_jobs=None):
        """The host default's result computed on the device (csrc/sparse_code.hip); n_jobs is
        ignored.  W may be RESIDENT.  The counters of the call land in ``sparse_code_counts``;
        like scikit-learn, one ConvergenceWarning when a row skipped a degenerate regressor or
        stopped early.  Rows in HBM (``is_device_array``) are coded where they lie, chunk by chunk, and the
        result is an array on their device that the coder writes itself (dbgsom_ctx_sparse_code_device)."""
        rows = self._query_rows(X, "sparse coding")
        if W is RESIDENT:
            self._require_loaded()
            keep, p, M = None, None, self._get("prototypes")
            d = self._d
        else:
            keep = np.ascontiguousarray(W, dtype=np.float64)
            if keep.ndim != 2:
                raise ValueError("W must be 2-D")
            p, (M, d) = keep.ctypes.data, keep.shape
        if rows.d != d:
            raise ValueError("prototype / sample feature mismatch")
        counts = np.zeros(len(_native.SC_COUNTS), dtype=np.uint64)
        if P is None:
            Pc, C = None, 0
        else:
            Pc = np.ascontiguousarray(P, dtype=np.float64)
            if Pc.ndim != 2 or Pc.shape[0] != M:
                raise ValueError("P must have one row per prototype")
            C = Pc.shape[1]
        out = rows.empty((rows.N, M if P is None else C), "float64")
        # (rows that are none go as a null pointer, and for rows in HBM so does their output)
        out_p = rows.ptr(out) if rows.N or rows.suffix == HOST else None
        self._query("sparse_code", "euclidean", rows, p, M, int(max_iter), None if Pc is None else Pc.ctypes.data, C,
                    out_p if P is None else None, None if P is None else out_p, counts.ctypes.data, null_when_empty=True)
        self.sparse_code_counts = dict(zip(_native.SC_COUNTS, (int(v) for v in counts)))
        if counts[4] or counts[5]:
            import warnings

            from sklearn.exceptions import ConvergenceWarning

            warnings.warn("sparse coding: %d degenerate regressor(s) skipped, %d early stop(s) of the LARS path "
                          "(scikit-learn warns the same way)" % (int(counts[4]), int(counts[5])),
                          ConvergenceWarning)
        return out

    # -- topographic function ---------------------------------------------------------------------
    def topographic_function(self, W, X, coords, want_distances=False):
        """The host default's result computed on the device (csrc/topofn.hip): the k = 2 search of
        ``bmu(W, 2, X=X)``, the edge set, a breadth-first search from every neuron and the histograms,
        with the pairs never leaving HBM.  Rows in HBM (``is_device_array``) are searched where they lie
        (dbgsom_ctx_topographic_function_device); the histograms are host arrays either way."""
        rows = self._query_rows(X, "topographic function")
        W64, M = self._w64(W, rows.d)
        xy = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 2)
        if xy.shape[0] != M:
            raise ValueError("coords must be (M, 2)")
        n_pos = int((xy.astype(np.int64).max(axis=0) - xy.astype(np.int64).min(axis=0)).max()) + 1
        hist_pos = np.empty(n_pos, dtype=np.int64)
        hist_neg = np.empty(M + 1, dtype=np.int64)
        D = np.empty((M, M), dtype=np.int32) if want_distances else None
        self._query("topographic_function", "euclidean", rows, W64.ctypes.data, M, round_f32(rows.dtype, W), xy.ctypes.data,
                    n_pos, hist_pos.ctypes.data, hist_neg.ctypes.data, None if D is None else D.ctypes.data)
        return hist_pos, hist_neg, D

    # -- a2 -------------------------------------------------------------------------------------
    def exp_similarity(self, distances, gamma):
        dd = np.ascontiguousarray(np.asarray(distances).reshape(-1), dtype=np.float64)
        out = np.empty_like(dd)
        self._call("dbgsom_ctx_exp_similarity", self._ctx, dd.ctypes.data, dd.size, float(gamma),
                   out.ctypes.data)
        return out

    # -- a5 / a6 --------------------------------------------------------------------------------
    def _topology(self, hop, M):
        # the estimator hands over the SAME array object until the lattice changes
        if hop is not self._hop_key:
            h = np.ascontiguousarray(hop, dtype=np.float64)
            if h.shape != (M, M):
                raise ValueError("hop matrix must be (M, M)")
            self._call("dbgsom_ctx_set_topology", self._ctx, h.ctypes.data, M)
            self._hop_key = hop

    # -- the epoch ------------------------------------------------------------------------------
    def epoch(self, W, hop, sigma, gamma, layout="compact", want_assignments=False,
              keep_on_device=False, n_classes=0, frozen=False):
        """One hot-path epoch (the body of BaseSom._grow_som, BaseSom.py:403-407) as ONE call of
        the C ABI.  `W` is a NumPy array or RESIDENT (the prototypes the previous epoch left in
        HBM); with `keep_on_device` the new prototypes stay in HBM (no PCIe round trip between
        epochs of a phase without growth) and only the O(M) statistics come back; `frozen`
        leaves the resident prototypes untouched (bench: the same map every step)."""
        self._require_loaded()
        keep, p, M, rf = self._w_arg(W)
        self._topology(hop, M)
        Wn = None if keep_on_device else np.empty((M, self._d))
        chg = np.empty(1)
        E = np.empty(M)
        a = np.empty(M)
        win = np.empty(self._N, dtype=np.int64) if want_assignments else None
        dist = np.empty(self._N) if want_assignments else None
        self._call("dbgsom_ctx_epoch", self._ctx, p, M, rf, float(gamma), float(sigma),
                   _native.LAYOUTS[layout], _native.EPOCH_FROZEN if frozen else 0,
                   None if Wn is None else Wn.ctypes.data, chg.ctypes.data, E.ctypes.data, a.ctypes.data,
                   None if win is None else win.ctypes.data, None if dist is None else dist.ctypes.data)
        self._last_M = M
        res = EpochResult(Wn, float(chg[0]), E, a, win, dist, RESIDENT if keep_on_device else None)
        if n_classes > 0:
            res.class_hist = self.class_histogram(None, n_classes, M)
        self._log_epoch()
        return res

    def epoch_masked(self, W, hop, sigma, gamma, want_assignments=False, n_classes=0):
        """One epoch on resident rows with missing entries as ONE call of the C ABI (csrc/masked.hip,
        csrc/masked_fit.hip, csrc/smooth.hip): dbgsom_ctx_epoch_masked."""
        self._require_loaded()
        if W is RESIDENT:
            raise ValueError("no prototypes stay resident between masked epochs")
        keep, p, M, _ = self._w_arg(W, d=self._d)
        self._topology(hop, M)
        Wn, chg, E, a = np.empty((M, self._d)), np.empty(1), np.empty(M), np.empty(M)
        want = want_assignments or n_classes > 0
        win = np.empty(self._N, dtype=np.int64) if want else None
        dist = np.empty(self._N) if want else None
        self._call("dbgsom_ctx_epoch_masked", self._ctx, p, M, float(gamma), float(sigma), Wn.ctypes.data,
                   chg.ctypes.data, E.ctypes.data, a.ctypes.data, None if win is None else win.ctypes.data,
                   None if dist is None else dist.ctypes.data)
        self._last_M = M
        res = EpochResult(Wn, float(chg[0]), E, a, win if want_assignments else None, dist if want_assignments else None)
        if n_classes > 0:
            res.class_hist = self.class_histogram(win, n_classes, M)
        return res

    def epoch_info(self):
        """dbgsom_ctx_epoch_info of the last epoch: [filtered (0/1), mean candidate-list length,
        digit planes (0 = no sweep), hinted (0/1), back-off epochs left, policy hold, mean list length
        of a counting-only pruning launch (NaN: none), full seed pre-pass (0/1)]."""
        info = (ctypes.c_double * 8)()
        _native.call("dbgsom_ctx_epoch_info", self._ctx, info)
        return [float(v) for v in info]

    def arm_ms(self):
        """dbgsom_ctx_arm_ms: {(seeds, planes): ms} of the arms of the search policy that have been timed."""
        ms = (ctypes.c_double * 12)()
        _native.call("dbgsom_ctx_arm_ms", self._ctx, ms)
        return {(i // 4, i % 4): float(v) for i, v in enumerate(ms) if v == v}

    def _log_epoch(self):
        info = self.epoch_info()
        if info[0]:
            self.filter_log.append(("filtered", float(info[1]), int(info[2])))
        elif self.algorithm != "exact":
            self.filter_log.append(("exact", None))
        del self.filter_log[:-64]
        if self.phase_log is not None:   # (needs the context option "timing")
            ms = (ctypes.c_double * 8)()
            _native.call("dbgsom_ctx_phase_ms", self._ctx, ms)
            self.phase_log.append([float(v) for v in ms])

    def update(self, W, hop, sigma, sample_weights, winners, distances, layout="compact"):
        """_update_weights + _write_accumulative_error with the caller's winners / sample weights
        (BaseSom.py:470-523, 541-561) -> (new_weights, change_total, errors, activations)."""
        self._require_loaded()
        keep, p, M, _ = self._w_arg(W)
        self._topology(hop, M)
        idx = np.ascontiguousarray(winners, dtype=np.int64)
        kw = np.ascontiguousarray(sample_weights, dtype=np.float64)
        dist = np.ascontiguousarray(distances, dtype=np.float64)
        if not (idx.size == kw.size == dist.size == self._N):
            raise ValueError("one winner / weight / distance per resident sample")
        Wn, chg, E, a = np.empty((M, self._d)), np.empty(1), np.empty(M), np.empty(M)
        self._call("dbgsom_ctx_update", self._ctx, p, M, idx.ctypes.data, kw.ctypes.data,
                   dist.ctypes.data, float(sigma), _native.LAYOUTS[layout], Wn.ctypes.data,
                   chg.ctypes.data, E.ctypes.data, a.ctypes.data)
        self._last_M = M
        return Wn, float(chg[0]), E, a

    def set_hint(self, winners, M):
        """Seeds of the next filtered search (any indices < M keep the result exact)."""
        idx = np.ascontiguousarray(winners, dtype=np.int64)
        if idx.size != self._N:
            raise ValueError("one seed per resident sample")
        self._call("dbgsom_ctx_set_hint", self._ctx, idx.ctypes.data, int(M))

    def read_sums(self, M):
        """The last epoch's reduced [S (M x d) | K | a | E] buffer."""
        out = np.empty(M * (self._d + 3))
        self._call("dbgsom_ctx_read_sums", self._ctx, out.ctypes.data, int(M))
        return out

    def filter_counts(self):
        """Candidate-list length per 128-sample workgroup of the last filtered search."""
        nb = (self._N + 127) // 128
        out = np.empty(nb, dtype=np.uint32)
        self._call("dbgsom_ctx_filter_counts", self._ctx, out.ctypes.data, nb)
        return out

    def read_anchors(self, aseed=False):
        """The anchor buckets of the resident samples (`anchor_state` 1): dict of `anchors` (A x padded features,
        chain order), `anchor_of` and `order` (one int32 per row) and, with `aseed`, the prototype the last search
        chose for every anchor (that search must have been seeded from the anchors)."""
        n = ctypes.c_int64(0)
        self._call("dbgsom_ctx_read_anchors", self._ctx, ctypes.byref(n), None, None, None, None)
        out = {"anchors": np.empty((n.value, self.padded_features)), "anchor_of": np.empty(self._N, dtype=np.int32),
               "order": np.empty(self._N, dtype=np.int32)}
        if aseed:
            out["aseed"] = np.empty(n.value, dtype=np.int32)
        self._call("dbgsom_ctx_read_anchors", self._ctx, None, out["anchors"].ctypes.data, out["anchor_of"].ctypes.data,
                   out["order"].ctypes.data, out["aseed"].ctypes.data if aseed else None)
        return out

    def read_anchor_runs(self):
        """The run table of the anchor buckets (`anchor_state` 1): dict of `run_start` (one int32 per 128-row workgroup
        of `order`, plus one) and per run `anchor`, `R` (>= the largest distance from a row of the run to its anchor) and
        `xx_max` (the largest squared norm of the run's rows)."""
        g = ctypes.c_int64(0)
        self._call("dbgsom_ctx_read_anchor_runs", self._ctx, ctypes.byref(g), None, None, None, None)
        cap = g.value + 256
        start = np.empty(g.value + 1, dtype=np.int32)
        anchor, R, xx = np.full(cap, -1, dtype=np.int32), np.full(cap, np.nan), np.full(cap, np.nan)
        self._call("dbgsom_ctx_read_anchor_runs", self._ctx, None, start.ctypes.data, anchor.ctypes.data, R.ctypes.data,
                   xx.ctypes.data)
        n = int(start[-1])
        return {"run_start": start, "anchor": anchor[:n], "R": R[:n], "xx_max": xx[:n]}

    def refine_counts(self):
        """[(sample, prototype) pairs evaluated exactly, 128-sample workgroups refined, samples whose
        candidates overflowed the four slots] of the last filtered search."""
        out = np.zeros(4, dtype=np.uint64)
        self._call("dbgsom_ctx_refine_counts", self._ctx, out.ctypes.data)
        return [int(v) for v in out]

    def traffic(self):
        """PCIe traffic of the prototypes since the context was created / last released."""
        keys = ("w_upload_calls", "w_upload_bytes", "w_download_calls", "w_download_bytes",
                "w_row_writes", "w_row_reads")
        return {k: self._get(k) for k in keys}

    _X_TRAFFIC = ("x_upload_bytes", "x_upload_calls", "x_download_bytes")

    def sample_traffic(self):
        """PCIe traffic of the samples since this backend was made (``release`` does not reset it):
        ``x_upload_bytes`` / ``x_upload_calls`` -- sample rows host -> HBM (``load``, every query handed over as a
        host array), ``x_download_bytes`` -- per-row results HBM -> host (winners, distances, codes, class
        probabilities, filled rows; ``fetch``).  Rows that are in HBM already (``load_device``, a device array
        as X) move neither."""
        return {k: self._x_traffic[k] + (self._get(k) if self._ctx else 0) for k in self._X_TRAFFIC}

    def plane_cost(self, p, mean, M):
        """Cost model of the engine's policy (csrc/search_policy.h, seeds = the previous winners) for `p` digit
        planes of the candidate sweep and candidate lists of `mean` entries; p = 0: no sweep, candidates from the
        triangle inequality (one pass over the top digit plane of X and an M x M matrix of prototype gaps)."""
        return self.arm_cost(p, mean, M, self._N, self.padded_features)

    @classmethod
    def arm_cost(cls, p, mean, M, N, dp):
        """plane_cost for N resident rows of dp padded features: SearchPolicy::model_cost(2, p, mean, M, N, dp),
        term for term (tests/test_search_policy_cpu.py holds the two together)."""
        if p == 0:
            launches = 25.0 / (2.8 * (float(max(N, 1)) * dp) / (1.0e6 * 784.0))
            return (cls.PRUNE_PASS_COST + cls.SWEEP_COST[1] * M * 9.0 * M / max(N, 1) + launches
                    + cls.LIST_COST * mean)
        return cls.SWEEP_COST[p] * M + cls.LIST_COST * mean

    # -- f-1 .. f-3: reductions that keep the N-sized arrays in HBM -----------------------------
    def column_moments(self):
        """(sum_i x_ij, sum_i (x_ij - mean_j)^2, N) over the resident samples in NumPy's axis-0
        arithmetic (sequential per column, X's dtype): np.var(X, 0) = s2 / N and
        np.std(X, 0, ddof=1) = sqrt(s2 / (N - 1)) bit for bit, without a host pass over X.
        None when the resident dtype has no NumPy counterpart (bfloat16)."""
        self._require_loaded()
        if isinstance(self._x_np_dtype, str) or self.resident_csr:
            return None
        s1 = np.empty(self._d, dtype=self._x_np_dtype)
        self._call("dbgsom_ctx_column_sums", self._ctx, None, s1.ctypes.data)
        mean = np.ascontiguousarray(np.true_divide(s1, self._N))
        s2 = np.empty_like(s1)
        self._call("dbgsom_ctx_column_sums", self._ctx, mean.ctypes.data, s2.ctypes.data)
        return s1, s2, self._N

    def covariance_apply(self, mean, V):
        """``HotPathBackend.covariance_apply`` on the resident rows (csrc/covariance.hip): mean, V up and Z, colsum
        down are all that crosses PCIe (2 d p + 2 d doubles)."""
        self._require_loaded()
        V64 = np.ascontiguousarray(V, dtype=np.float64)
        m64 = np.ascontiguousarray(mean, dtype=np.float64)
        if V64.ndim != 2 or V64.shape[0] != self._d or not 1 <= V64.shape[1] <= _native.MAX_DIRECTIONS:
            raise ValueError(f"V must be ({self._d}, p) with 1 <= p <= {_native.MAX_DIRECTIONS}, got {V64.shape}")
        if m64.shape != (self._d,):
            raise ValueError(f"mean must have shape ({self._d},), got {m64.shape}")
        Z = np.empty_like(V64)
        colsum = np.empty(self._d)
        self._call("dbgsom_ctx_covariance_apply", self._ctx, m64.ctypes.data, V64.ctypes.data, int(V64.shape[1]),
                   Z.ctypes.data, colsum.ctypes.data)
        return Z, colsum

    _weighted = False
    _incomplete = False

    def set_sample_weight(self, w):
        """One float64 weight per resident row, kept in HBM next to the samples (None detaches)."""
        self._require_loaded()
        super().set_sample_weight(w)
        if w is None:
            self._call("dbgsom_ctx_set_sample_weight", self._ctx, None, 0)
        else:
            self._call("dbgsom_ctx_set_sample_weight", self._ctx, self._sw.ctypes.data, self._sw.size)
        self._weighted = w is not None

    def weight_total(self) -> float:
        """Sum of the resident rows' weights (the number of rows when none are attached)."""
        out = np.empty(1)
        self._call("dbgsom_ctx_weight_total", self._ctx, out.ctypes.data)
        return float(out[0])

    def weighted_column_moments(self, total):
        """(sum_i w_i x_ij, sum_i w_i (x_ij - mean_j)^2) over the resident samples, mean = the first over
        `total` (the summed weight): accumulated in float64 whatever the storage dtype."""
        self._require_loaded()
        s1 = np.empty(self._d)
        self._call("dbgsom_ctx_weighted_column_sums", self._ctx, None, s1.ctypes.data)
        mean = np.ascontiguousarray(s1 / total)
        s2 = np.empty(self._d)
        self._call("dbgsom_ctx_weighted_column_sums", self._ctx, mean.ctypes.data, s2.ctypes.data)
        return s1, s2

    # (rows with missing entries, metric="manhattan" / "cosine": the O(N)-per-fit reductions are HotPathBackend's host
    #  defaults over the masked bmu / the bmu of that metric)
    def quantization_error(self, W) -> float:
        self._require_loaded()
        if self._incomplete or self._other_metric:
            return super().quantization_error(W)
        keep, p, M, rf = self._w_arg(W)
        out = np.empty(2)
        self._call("dbgsom_ctx_quantization_error", self._ctx, p, M, rf, out.ctypes.data)
        return float(out[0] / out[1])

    def topographic_error_count(self, W, coords) -> int:
        self._require_loaded()
        if self._incomplete or self._other_metric:
            return super().topographic_error_count(W, coords)
        keep, p, M, rf = self._w_arg(W)
        xy = np.ascontiguousarray(coords, dtype=np.int32)
        if xy.shape != (M, 2):
            raise ValueError("coords must be (M, 2)")
        out = np.empty(1)
        self._call("dbgsom_ctx_topographic_count", self._ctx, p, M, rf, xy.ctypes.data, out.ctypes.data)
        return float(out[0]) if self._weighted else int(round(out[0]))

    def node_statistics(self, W, sigma):
        """-> (hit_counts (M,), density_sums (M,)) of BaseSom._calculate_node_statistics."""
        self._require_loaded()
        if self._incomplete or self._other_metric:
            return super().node_statistics(W, sigma)
        keep, p, M, rf = self._w_arg(W)
        hits, dens = np.empty(M), np.empty(M)
        self._call("dbgsom_ctx_node_statistics", self._ctx, p, M, rf, float(sigma), hits.ctypes.data,
                   dens.ctypes.data)
        return hits, dens

    def set_labels(self, y):
        super().set_labels(y)
        if y is None:
            self._call("dbgsom_ctx_set_labels", self._ctx, None, 0)
        else:
            self._call("dbgsom_ctx_set_labels", self._ctx, self._y.ctypes.data, self._y.size)

    def class_histogram(self, winners, n_classes, M):
        """(M, n_classes) int64 over all ranks (float64 summed weights with weights attached);
        winners=None: the last epoch's (still in HBM)."""
        if self._incomplete or self._other_metric:
            return super().class_histogram(winners, n_classes, M)
        idx = None if winners is None else np.ascontiguousarray(winners, dtype=np.int64)
        if self._weighted:
            hist = np.empty((M, n_classes), dtype=np.float64)
            self._call("dbgsom_ctx_class_histogram_weighted", self._ctx, None if idx is None else idx.ctypes.data,
                       int(n_classes), int(M), hist.ctypes.data)
            return hist
        hist = np.empty((M, n_classes), dtype=np.int64)
        self._call("dbgsom_ctx_class_histogram", self._ctx, None if idx is None else idx.ctypes.data,
                   int(n_classes), int(M), hist.ctypes.data)
        return hist

    # -- per-unit statistics of a per-row quantity (csrc/unit_sums.hip) ----------------------------------
    def _unit_fold_host(self, units, Z, w, M):
        mass, sums = np.empty(M), np.empty((M, Z.shape[1]))
        self._call("dbgsom_ctx_unit_sums", self._ctx, units.ctypes.data, Z.ctypes.data, None if w is None else w.ctypes.data,
                   units.size, int(M), Z.shape[1], mass.ctypes.data, sums.ctypes.data)
        return mass, sums

    def _unit_fold_device(self, units, Z, w, M):
        V = int(Z.shape[1])
        mass, sums = device_empty(Z, (M,), "float64"), device_empty(Z, (M, V), "float64")
        self._producer_done(Z)
        self._call("dbgsom_ctx_unit_sums_device", self._ctx, ctypes.c_void_p(units.data_ptr()),
                   ctypes.c_void_p(Z.data_ptr()), int(Z.stride(0)) if Z.shape[0] > 1 else V,
                   None if w is None else ctypes.c_void_p(w.data_ptr()), int(Z.shape[0]), int(M), V,
                   ctypes.c_void_p(mass.data_ptr()), ctypes.c_void_p(sums.data_ptr()), V)
        return mass, sums

    def _unit_deviations_device(self, units, Y, C, mode):
        N, V = int(Y.shape[0]), int(Y.shape[1])
        out = device_empty(Y, (N, V) if mode == DEVIATIONS_SQUARES else (N, 1), "float64")
        self._producer_done(Y)
        self._call("dbgsom_ctx_unit_deviations_device", self._ctx, ctypes.c_void_p(units.data_ptr()),
                   ctypes.c_void_p(Y.data_ptr()), int(Y.stride(0)) if N > 1 else V, N, ctypes.c_void_p(C.data_ptr()), V,
                   int(C.shape[0]), V, int(mode), ctypes.c_void_p(out.data_ptr()), V)
        return out

    def _unit_device_arg(self, a, like, dtype, what):
        """`a` as a contiguous array of `dtype` next to `like`: host arrays go up with ``put``"""
        if a is None:
            return None
        if not is_device_array(a):
            return self.put(np.ascontiguousarray(a, dtype=dtype), like)
        if dtype_name(a) != dtype:
            raise ValueError(f"{what} on the device must be {dtype}, got {dtype_name(a)}")
        index = getattr(a.device, "index", None)
        if index is not None and index != self.device_index:
            raise ValueError(f"{what} lives on GPU {index}, this backend runs on GPU {self.device_index}")
        return a.contiguous()

    def unit_statistics(self, units, Y, w, M, want_std=False, want_err=False):
        """The folds on the device (csrc/unit_sums.hip).  Host arrays: units, Y and w go up and M x (1 + V) doubles
        come down per fold (dbgsom_ctx_unit_sums); the deviations between two folds are elementwise NumPy.  With
        units, Y or w on this backend's device everything stays there (dbgsom_ctx_unit_sums_device,
        dbgsom_ctx_unit_deviations_device; arguments given on the host are moved with ``put``) and the results
        are arrays on that device."""
        M = int(M)
        if not 1 <= M <= _native.MAX_PROTOTYPES:
            raise ValueError(f"M must be 1 .. {_native.MAX_PROTOTYPES}, got {M}")
        like = next((a for a in (Y, units, w) if a is not None and is_device_array(a)), None)
        if like is None:
            units, Y, w = _unit_args(units, Y, w)
            mass, sums = self._unit_fold_host(units, Y, w, M)
            with np.errstate(all="ignore"):
                mean = sums / mass[:, None]
                std = err = None
                if want_std:
                    m2, sq = self._unit_fold_host(units, unit_deviations(units, Y, mean, DEVIATIONS_SQUARES), w, M)
                    std = np.sqrt(sq / m2[:, None])
                if want_err:
                    dev = np.ascontiguousarray(unit_deviations(units, Y, mean, DEVIATIONS_NORM)[:, None])
                    err = self._unit_fold_host(units, dev, w, M)[1][:, 0]
            return mass, mean, std, err
        units = self._unit_device_arg(units, like, "int64", "units").reshape(-1)
        Y = self._unit_device_arg(Y, like, "float64", "the values")
        Y = Y.reshape(int(units.shape[0]), -1)
        w = self._unit_device_arg(w, like, "float64", "the weights")
        if not 1 <= int(Y.shape[1]) <= _native.MAX_MIXTURE_VALUES:
            raise ValueError(f"1 .. {_native.MAX_MIXTURE_VALUES} values per row, got {int(Y.shape[1])}")
        if w is not None and tuple(w.shape) != tuple(units.shape):
            raise ValueError("one weight per row")
        ns = array_namespace(like)
        mass, sums = self._unit_fold_device(units, Y, w, M)
        mean = sums / mass[:, None]
        std = err = None
        if want_std:
            m2, sq = self._unit_fold_device(units, self._unit_deviations_device(units, Y, mean, DEVIATIONS_SQUARES), w, M)
            std = ns.sqrt(sq / m2[:, None])
        if want_err:
            err = self._unit_fold_device(units, self._unit_deviations_device(units, Y, mean, DEVIATIONS_NORM), w, M)[1][:, 0]
        return mass, mean, std, err

    def set_targets(self, Y):
        """float64 targets (N x V) of the resident rows, copied next to them in HBM (a host array or an array on this
        device); None detaches."""
        if Y is None:
            super().set_targets(None)
            self._call("dbgsom_ctx_set_targets", self._ctx, None, 0, 0)
            self._targets_attached = False
            return
        self._require_loaded()
        if is_device_array(Y):
            Yd = self._unit_device_arg(Y, Y, "float64", "the targets")
            Yd = Yd.reshape(int(Yd.shape[0]), -1)
            self._producer_done(Yd)
            self._call("dbgsom_ctx_set_targets_device", self._ctx, ctypes.c_void_p(Yd.data_ptr()), int(Yd.shape[0]),
                       int(Yd.shape[1]), int(Yd.shape[1]))
            self._targets = Y     # (the host fallback of target_statistics fetches it when it is needed)
        else:
            super().set_targets(Y)
            self._call("dbgsom_ctx_set_targets", self._ctx, self._targets.ctypes.data, self._targets.shape[0],
                       self._targets.shape[1])
        self._targets_attached = True

    _targets_attached = False

    def target_statistics(self, winners, M, want_std=False, want_err=False):
        """-> (mass, mean, std | None, err | None) of the attached targets per unit, host arrays
        (dbgsom_ctx_target_statistics); winners=None: the last epoch's (still in HBM)."""
        if self._incomplete or self._other_metric:
            if is_device_array(self._targets):
                self._targets = self.fetch(self._targets).reshape(self._N, -1)
            return super().target_statistics(winners, M, want_std, want_err)
        if not self._targets_attached:
            raise RuntimeError("no targets attached: call set_targets(Y) first")
        M, V = int(M), int(self._targets.shape[1]) if len(self._targets.shape) > 1 else 1
        idx = None if winners is None else np.ascontiguousarray(winners, dtype=np.int64)
        mass, mean = np.empty(M), np.empty((M, V))
        std = np.empty((M, V)) if want_std else None
        err = np.empty(M) if want_err else None
        self._call("dbgsom_ctx_target_statistics", self._ctx, None if idx is None else idx.ctypes.data, M, mass.ctypes.data,
                   mean.ctypes.data, None if std is None else std.ctypes.data, None if err is None else err.ctypes.data)
        return mass, mean, std, err

    # -- vertical growth on Voronoi subsets (f-4) -------------------------------------------------
    def partition(self, W, want_winners=False):
        """BMU of every resident sample + bucket order -> (samples per neuron, winners | None)."""
        self._require_loaded()
        keep, p, M, rf = self._w_arg(W)
        counts = np.empty(M, dtype=np.int64)
        win = np.empty(self._N, dtype=np.int64) if want_winners else None
        self._call("dbgsom_ctx_partition", self._ctx, p, M, rf, counts.ctypes.data,
                   None if win is None else win.ctypes.data)
        self._part_M = M
        return counts, win

    def read_partition(self):
        """The bucket order ``partition`` left on the device -> (order (rows,) int32, seg_start (units + 1,) uint32):
        unit j's rows are ``order[seg_start[j]:seg_start[j + 1]]``, ascending."""
        self._require_loaded()
        M = int(self._part_M)
        order, seg = np.empty(self._N, dtype=np.int32), np.empty(M + 1, dtype=np.uint32)
        self._call("dbgsom_ctx_read_partition", self._ctx, order.ctypes.data, seg.ctypes.data)
        return order, seg

    # -- the nearest resident rows of a query, through the partition -----------------------------------
    def row_neighbors(self, W, k, n_probe, Q):
        """The k nearest resident rows among those filed under a row's n_probe nearest units
        (csrc/kneighbors.hip, then csrc/row_neighbors.hip): the unit search of a chunk leaves its probe lists on the
        device and one workgroup per row scans the rows ``partition`` filed under them.  Host rows go up in chunks
        of ``distances_chunk_rows`` rows and rows x k x 16 bytes come down; for rows in HBM both results are arrays on
        their device that the kernel writes itself (dbgsom_ctx_row_neighbors_query_device).  Dense float32 /
        float64 residents only."""
        self._require_loaded()
        rows = self._query_rows(Q, "row_neighbors", defer=True)
        W64, M = self._w64(W, rows.d)
        k, n_probe = int(k), int(n_probe)
        check_row_neighbors(k, n_probe, M)
        if rows.d != self._d:
            raise ValueError(f"Q has {rows.d} features, the resident rows {self._d}")
        if rows.d > _native.MAX_SCAN_FEATURES:
            raise ValueError(f"rows of more than DBGSOM_MAX_SCAN_FEATURES = {_native.MAX_SCAN_FEATURES} features are "
                             f"not scanned, got {rows.d}")
        dist, idx = rows.empty((rows.N, k), "float64"), rows.empty((rows.N, k), "int64")
        if rows.N:
            try:
                self._query("row_neighbors_query", "euclidean", rows, W64.ctypes.data, M, n_probe, k, rows.ptr(idx),
                            rows.ptr(dist))
            except _native.DbgsomNativeError as e:
                if e.code == -4:   # DBGSOM_ESTATE: the message says what is missing
                    raise ValueError(f"{e}: call partition(W) on dense float32 / float64 residents first") from None
                raise
        return dist, idx

    def subset(self, neuron):
        """A backend whose resident samples are the Voronoi set of `neuron` (gathered in HBM)."""
        child = ctypes.c_void_p()
        self._call("dbgsom_ctx_subset_create", self._ctx, int(neuron), ctypes.byref(child))
        sub = HipBackend(self.device_index, self.algorithm, _ctx=child)
        sub._weighted = self._weighted   # (dbgsom_ctx_subset_create gathered the rows' weights)
        return sub

    _SETTABLE = ("algorithm", "sweep_planes", "seed_stride", "timing", "refine", "filter_min_query_rows",
                 "max_mean_candidates", "shard_smooth", "csr_densify_below", "anchor_seeds")

    def release(self):
        """Give the device memory back (the backend can be loaded again afterwards; options stay)."""
        if self._ctx:
            opts = {k: self._get(k) for k in self._SETTABLE}
            for k in self._X_TRAFFIC:
                self._x_traffic[k] += self._get(k)
            _native.call("dbgsom_ctx_destroy", self._ctx)
            self._ctx = ctypes.c_void_p()
            _native.call("dbgsom_ctx_create", self.device_index, ctypes.byref(self._ctx))
            for k, v in opts.items():
                self._set(k, v)
            self._install_collective()
        self._loaded = False
        self.resident_serial += 1
        self._borrowed = None
        self._hop_key = None
        self._weighted = False
        self._incomplete = False
        self._metric = "euclidean"
        self._sw = None
        self._targets = None
        self._targets_attached = False

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                self._lib.dbgsom_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:  # interpreter shutdown
            pass
