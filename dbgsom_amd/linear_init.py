"""Linear initialisation (``init="pca"``): the plane of the first two principal directions of the resident rows,
found by a block subspace iteration with Rayleigh-Ritz, and the start prototypes laid out on it.

Backend-agnostic: the only thing asked of the engine is ``covariance_apply(mean, V) -> (Z, colsum)`` with
``Z = C^T (C V)``, ``C = X - mean`` and ``colsum = sum_i C_i`` over the resident rows (``csrc/covariance.hip`` on the
GPU).  Everything else is d x p host arithmetic in float64, p = min(8, d).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

BLOCK = 8            # columns of the iterated block (DBGSOM_MAX_DIRECTIONS)
MAX_PASSES = 60
RESIDUAL_TOL = 1e-8  # stop when max_j ||r_j|| <= RESIDUAL_TOL * theta_1
SEED = 12345         # of the fixed start block: the run is deterministic


class PrincipalPlane(NamedTuple):
    mean: np.ndarray         # (d,)   column means
    directions: np.ndarray   # (2, d) unit eigenvectors of the covariance, largest eigenvalue first, signs fixed
    variances: np.ndarray    # (2,)   their eigenvalues (population covariance, divisor N)
    n_passes: int            # covariance passes the iteration took (the pass for the mean not counted)
    residual: float          # max_j ||r_j|| / theta_1 at the last pass


def fix_sign(v: np.ndarray) -> np.ndarray:
    """v or -v: the entry of largest magnitude positive (lowest index on ties)."""
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def principal_plane(engine, n_rows: int, d: int) -> PrincipalPlane:
    """The two leading principal directions of the engine's resident rows (n_rows x d)."""
    if d < 2:
        raise ValueError('init="pca" needs at least two features: X has fewer than two directions of variance')
    p = min(BLOCK, d)
    V = np.linalg.qr(np.random.default_rng(SEED).normal(size=(d, p)))[0]
    V = np.ascontiguousarray(V, dtype=np.float64)
    _, colsum = engine.covariance_apply(np.zeros(d), V)
    mean = np.asarray(colsum, dtype=np.float64) / n_rows
    passes, rel = 0, np.inf
    theta = np.zeros(2)
    U = V[:, :2]
    while True:
        Z, _ = engine.covariance_apply(mean, V)
        passes += 1
        if not np.isfinite(Z).all():
            raise ValueError('init="pca": the covariance of X is not finite (NaN or infinity in X, or overflow)')
        B = V.T @ Z
        B = 0.5 * (B + B.T)
        lam, S = np.linalg.eigh(B)
        S2 = S[:, ::-1][:, :2]                      # the two leading Ritz vectors in the block's coordinates
        theta = lam[::-1][:2]
        U = V @ S2
        R = Z @ S2 - U * theta[None, :]
        if not theta[0] > 0:
            break                                   # (no variance at all: refused by the caller)
        rel = float(np.linalg.norm(R, axis=0).max() / theta[0])
        if rel <= RESIDUAL_TOL or passes >= MAX_PASSES:
            break
        V = np.ascontiguousarray(np.linalg.qr(Z)[0])
    variances = theta / n_rows
    if not variances[1] > 0:
        raise ValueError('init="pca": X has fewer than two directions of variance (the second eigenvalue of its '
                         f"covariance is {variances[1]!r}, not > 0)")
    directions = np.stack([fix_sign(U[:, j] / np.linalg.norm(U[:, j])) for j in range(2)])
    return PrincipalPlane(mean, directions, np.array(variances, dtype=np.float64), passes, rel)


def grid_prototypes(plane: PrincipalPlane, rows: int, cols: int) -> np.ndarray:
    """Prototype (a, b), row-major: mean + (2a/(rows-1) - 1) sqrt(l1) e1 + (2b/(cols-1) - 1) sqrt(l2) e2, float64."""
    a = 2.0 * np.arange(rows, dtype=np.float64) / (rows - 1) - 1.0
    b = 2.0 * np.arange(cols, dtype=np.float64) / (cols - 1) - 1.0
    s1, s2 = np.sqrt(plane.variances[0]), np.sqrt(plane.variances[1])
    e1, e2 = plane.directions
    W = (plane.mean[None, None, :] + (a * s1)[:, None, None] * e1[None, None, :]
         + (b * s2)[None, :, None] * e2[None, None, :])
    return np.ascontiguousarray(W.reshape(rows * cols, -1))
