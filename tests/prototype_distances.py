"""Helpers of the prototype_distances tests (tests/test_prototype_distances_cpu.py, tests/test_gpu_prototype_distances.py):
the oracle matrix, the shape tables of the raw device calls, the launcher of csrc/distances.hip restated, and a CPU
stand-in backend.

The oracle is oracle/bmu_chain.c as it is: column j of the matrix is the search's distance to a map that holds
prototype j alone, so every entry's bits are those the search would report for that pair."""
import functools

import numpy as np

from oracle import som_oracle as o
from tests import device_abi as da
from tests.test_missing_cpu import MaskedOracleBackend, masked_distances

SENTINEL = -1234.5     # what the output buffers are filled with: no distance is negative


# ---- oracle -------------------------------------------------------------------------------------------------------
def pair_distances(X, W):
    """(N x M) float64.  Complete rows: column j = oracle.bmu_chain(X, W[j:j+1], 1)[0]; bfloat16 bit patterns
    (uint16) are widened first; rows with NaN: tests.test_missing_cpu.masked_distances."""
    X = da.widen(np.asarray(X))
    W = np.ascontiguousarray(W, dtype=np.float64)
    out = np.empty((X.shape[0], W.shape[0]), dtype=np.float64)
    holes = np.isnan(X).any(axis=1)
    if holes.any():
        out[holes] = masked_distances(X[holes], W)
    if not holes.all():
        Xc = np.ascontiguousarray(X[~holes])
        cols = np.empty((W.shape[0], Xc.shape[0]), dtype=np.float64)
        for j in range(W.shape[0]):
            cols[j] = o.bmu_chain(Xc, W[j:j + 1], 1)[0]
        out[~holes] = cols.T
    return out


# ---- shape table of dbgsom_distances -------------------------------------------------------------------------------
# (dtype, N, M, d, pad, x_off, ldo_pad, out_off): ldx = d + pad, row 0 of X x_off elements into its allocation,
# ldo = M + ldo_pad, the result out_off * 8 bytes into its (256-byte aligned) allocation.  Pairwise, not a product:
# every value of a dimension occurs, and every form of the launcher for both float types.
N_VALUES = [1, 127, 128, 129, 300]
M_VALUES = [1, 5, 31, 32, 33, 64, 100, 129, 260]
D_VALUES = [1, 3, 16, 17, 48, 784]
CASES = [
    # LDS-DMA form: d % 16 == 0, aligned rows
    ("f32", 300, 5, 16, 0, 0, 0, 0), ("f32", 129, 64, 48, 0, 0, 3, 0), ("f32", 128, 100, 784, 0, 0, 0, 1),
    ("f32", 127, 260, 16, 0, 0, 3, 1), ("f32", 1, 129, 48, 0, 0, 0, 0), ("f32", 300, 33, 784, 0, 0, 3, 0),
    ("f32", 300, 32, 32, 4, 0, 0, 0),
    ("f64", 300, 31, 48, 0, 0, 3, 0), ("f64", 129, 100, 16, 0, 0, 0, 0), ("f64", 127, 260, 784, 0, 0, 0, 1),
    ("f64", 128, 32, 16, 0, 0, 3, 1), ("f64", 300, 64, 32, 2, 0, 0, 0),
    # register-staged form: any d, strided and unaligned rows, bfloat16
    ("f32", 1, 1, 1, 0, 0, 0, 0), ("f32", 127, 5, 3, 3, 0, 3, 0), ("f32", 129, 33, 17, 0, 1, 0, 1),
    ("f32", 300, 260, 17, 3, 0, 3, 1), ("f32", 128, 129, 16, 3, 0, 0, 0),
    ("f64", 300, 1, 3, 3, 0, 3, 1), ("f64", 127, 31, 17, 0, 0, 0, 0), ("f64", 129, 64, 1, 3, 0, 3, 0),
    ("f64", 1, 260, 48, 3, 0, 0, 1), ("f64", 128, 100, 784, 3, 0, 0, 0),
    ("bf16", 300, 100, 16, 0, 0, 0, 0), ("bf16", 129, 129, 784, 0, 0, 3, 1), ("bf16", 127, 32, 3, 3, 1, 0, 0),
    ("bf16", 128, 5, 48, 3, 0, 3, 0), ("bf16", 1, 33, 17, 0, 0, 0, 1),
]
CASE_IDS = ["%s-N%d-M%d-d%d-pad%d-xoff%d-ldo+%d-ooff%d" % c for c in CASES]

# dbgsom_distances_masked: make_case shapes of tests/test_missing_cpu.py.  The last one reaches the 16-row store kernel
# (N >= 8192), rooted and squared: a last workgroup with one row, a feature tail behind one step of four, one
# prototype block
MASKED_SHAPES = [(7, 3, 2), (257, 17, 5), (1000, 64, 129), (8192 + 17, 5, 3)]
MASKED_FRACS = [0.3, 0.9]


def launcher_form(case):
    """-> ('dma', chunk tiles 1 | 2 | 4) or ('reg',): the kernel launch_distances picks (csrc/distances.hip: the
    dispatch of launch_bmu; W is contiguous and 16-byte aligned here), and whether it stores 16 bytes at a time"""
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    form = da.bmu_class(dtype, d, d + pad, x_off, 0, M)
    return (form[:2] if form[0] == "dma" else ("reg",)), (out_off % 2 == 0 and (M + ldo_pad) % 2 == 0)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> (X as stored, W, D): the inputs of a table entry and the oracle's matrix, computed once and shared (read
    only).  With M >= 3 the last prototype duplicates the first, and prototype M // 2 is row N // 2 of X."""
    dtype, N, M, d, pad, x_off, ldo_pad, out_off = case
    rng = np.random.default_rng(1000 * N + 10 * M + d + len(dtype))
    X = da.stored(rng.normal(size=(N, d)) * rng.uniform(0.5, 3.0, size=d), dtype)
    W = rng.normal(size=(M, d)) * 1.5
    if M >= 3:
        W[M - 1] = W[0]
        W[M // 2] = da.widen(X)[N // 2].astype(np.float64)
    D = pair_distances(X, W)
    for a in (X, W, D):
        a.setflags(write=False)
    return X, W, D


# ---- CPU stand-in backend --------------------------------------------------------------------------------------------
class DistancesOracleBackend(MaskedOracleBackend):
    """MaskedOracleBackend with ``distances`` / ``distances_masked`` from the oracle (TESTS ONLY); records the rows
    of every call."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.distance_rows, self.masked_distance_rows = [], []

    def distances(self, W, X):
        if hasattr(X, "toarray"):
            X = X.toarray()
        X = np.ascontiguousarray(X)
        assert not np.isnan(X).any()
        self.distance_rows.append(len(X))
        return pair_distances(X, W)

    def distances_masked(self, W, X):
        assert np.isnan(X).any(axis=1).all()
        self.masked_distance_rows.append(len(X))
        return masked_distances(X, W)
