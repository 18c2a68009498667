"""Planted inputs for the sparse-coding tests and a row-level scikit-learn reference (test helper, no
tests here).

`planted` builds maps and queries whose non-negative LARS-lasso path is long (large final supports,
many drops) yet well conditioned; `reference` is the call csrc/sparse_code.hip restates
(DESIGN.md 4b), row by row, so that it also returns the iteration counts that SparseCoder hides.
tests/test_sparse_code_inputs_cpu.py proves, with the reference alone, that every case below meets the
conditions tests/test_gpu_sparse_code_paths.py relies on."""
import itertools
import warnings
from functools import lru_cache

import numpy as np

# DESIGN.md 4b "Parity rule": max |dcode| against scikit-learn, by query dtype
GATE = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-6}
# scikit-learn against itself under a feature permutation must stay below 1/100 of the gate
SELF_NOISE = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-8}

SC_CAP = 64     # csrc/sparse_code.hip: active-set cap of the LDS path
SC_CAP1 = 192   # ... of the first overflow pass


def normalize(A):
    from sklearn.preprocessing import normalize as sk_normalize

    return sk_normalize(A)


def planted(d, M, s, n, noise, seed):
    """W = |N(0,1)| + 0.1 N(0,1) (M x d); each of the n queries is a positive combination (weights
    uniform in [0.5, 1.5]) of s random rows of normalize(W) plus noise N(0,1).  float64 arrays.

    noise must be positive: the noiseless form leaves coefficients sitting on zero, and scikit-learn
    then moves against itself (under a feature permutation) by more than the parity gates allow."""
    if not noise > 0:
        raise ValueError("planted inputs need noise > 0")
    rng = np.random.default_rng(seed)
    W = np.abs(rng.normal(size=(M, d))) + 0.1 * rng.normal(size=(M, d))
    Wn = normalize(W)
    return W, plant_queries(Wn, s, n, noise, rng)


def plant_queries(Wn, s, n, noise, rng):
    """n queries planted on the normalised map Wn (see `planted`)."""
    M, d = Wn.shape
    X = np.empty((n, d))
    for i in range(n):
        rows = rng.choice(M, size=s, replace=False)
        X[i] = rng.uniform(0.5, 1.5, size=s) @ Wn[rows] + noise * rng.normal(size=d)
    return X


def f32_queries(X):
    """The float32 form of planted queries: every row rounded to a power-of-two grid of its own, coarse
    enough that its float32 sum of squares is exact in any summation order (integers n_k = x_k / grid
    with sum n_k^2 < 2^24).  sklearn's float32 normalize is then bit-identical under a feature
    permutation.  Without this a permutation changes the float32 norm by an ulp on most rows, every
    element of normalize(X) is rounded anew, and scikit-learn moves against itself by 3e-8 ... 1.5e-7
    on the cases below: that would measure the float32 rounding of the input, not the path."""
    X = np.asarray(X, dtype=np.float64)
    amax = np.abs(X).max(axis=1, keepdims=True)
    amax[amax == 0] = 1.0
    grid = 2.0 ** np.ceil(np.log2(amax * np.sqrt(X.shape[1]) / 4095.0))
    Q = (np.rint(X / grid) * grid).astype(np.float32)
    n = Q.astype(np.float64) / grid
    assert np.array_equal(n, np.rint(n)) and ((n * n).sum(axis=1) < 2.0 ** 24).all()
    return Q


def queries(X, dtype):
    return f32_queries(X) if np.dtype(dtype) == np.float32 else np.ascontiguousarray(X, dtype=np.float64)


def reference(W, X, max_iter=1000):
    """Per row: lars_path_gram(Xy, Gram, n_samples=d, method="lasso", positive=True, alpha_min=0) on
    normalize(W), normalize(X), the query dtype kept through normalize as SparseCoder does.  Gram and
    Cov are formed as SparseCoder forms them.  Returns (codes, iterations per row); any warning is
    an error."""
    from sklearn.linear_model import lars_path_gram

    W = np.asarray(W, dtype=np.float64)
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    Wn, Xn = normalize(W), normalize(X)
    gram = np.dot(Wn, Wn.T)
    cov = np.dot(Wn, Xn.T)
    code = np.zeros((X.shape[0], W.shape[0]))
    iters = np.zeros(X.shape[0], dtype=np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for i in range(X.shape[0]):
            _, _, coef, n_iter = lars_path_gram(Xy=cov[:, i], Gram=gram, n_samples=W.shape[1], method="lasso",
                                                positive=True, alpha_min=0, max_iter=max_iter, return_path=False,
                                                return_n_iter=True)
            code[i] = coef
            iters[i] = n_iter
    return code, iters


def permuted(W, X, seed=12345):
    """The same problem with the feature columns of W and X permuted together."""
    p = np.random.default_rng(seed).permutation(W.shape[1])
    return np.ascontiguousarray(W[:, p]), np.ascontiguousarray(X[:, p])


# ---------------------------------------------------------------------------------------------------
# the cases: name -> (d, M, s, rows, noise, seed).  Seeds were chosen on the CPU, by the reference
# alone, so that every case meets the conditions of tests/test_sparse_code_inputs_cpu.py
# ---------------------------------------------------------------------------------------------------
CASES = {
    "pass1": (256, 300, 60, 64, 0.01, 101),         # final supports in (64, 192]: the first overflow pass
    "pass2": (512, 400, 250, 64, 0.01, 101),        # final supports > 192: the second overflow pass
    "pass2_big": (784, 1030, 230, 16, 0.005, 101),  # ... with slots of cap 1000, iterations near max_iter
    "wide": (64, 200, 10, 12, 0.01, 107),           # M > d with the support well below d
}
# "pass2" is a mixed call: after its own rows, rows of (s, count) planted on the same map, all shuffled,
# so that the LDS path (s = 5), the first pass (s = 60) and the second pass (s = 250) have work in one call
PASS2_EXTRA = ((5, 6), (60, 6))

# cap boundaries: d = M + 3 and s = M, every prototype ends active, so the `na >= M` stop fires at, one
# below and one above each cap.  These nearly square systems are the worst conditioned of the cases
# (scikit-learn against itself: 1e-13 ... 6e-13), hence few rows and chosen seeds
BOUNDARY = {63: 264, 64: 264, 65: 265, 191: 435, 192: 417, 193: 457}   # M -> seed
BOUNDARY_ROWS = 3
for _m, _seed in BOUNDARY.items():
    CASES["all_active_%d" % _m] = (_m + 3, _m, _m, BOUNDARY_ROWS, 0.01, _seed)

# rows of the float32 form of a case (default: all); the reference takes 0.3 s ... 2 s per row on these
F32_ROWS = {"pass2": 32, "pass2_big": 8}

MAX_ITERS = (0, 1, 5, 64, 65, 192, 193)   # on the first rows of "pass1"; some of them take more iterations
MAX_ITER_ROWS = 8


@lru_cache(maxsize=None)
def case(name):
    """(W, X, s per row) of a case, float64, read-only."""
    d, M, s, n, noise, seed = CASES[name]
    W, X = planted(d, M, s, n, noise, seed)
    kind = np.full(n, s)
    if name == "pass2":
        Wn = normalize(W)
        for j, (s2, n2) in enumerate(PASS2_EXTRA):
            X = np.vstack([X, plant_queries(Wn, s2, n2, noise, np.random.default_rng(seed + 1000 + j))])
            kind = np.concatenate([kind, np.full(n2, s2)])
        order = np.random.default_rng(seed + 2000).permutation(X.shape[0])
        X, kind = np.ascontiguousarray(X[order]), kind[order]
    for a in (W, X, kind):
        a.setflags(write=False)
    return W, X, kind


def case_queries(name, dtype):
    """The case's queries in `dtype` (float32: the first F32_ROWS) and their s per row."""
    _, X, kind = case(name)
    n = F32_ROWS.get(name, X.shape[0]) if np.dtype(dtype) == np.float32 else X.shape[0]
    return queries(X[:n], dtype), kind[:n]


def support_range(name, s):
    """The inclusive range of final support sizes that the GPU tests rely on, for rows planted with s."""
    M = CASES[name][1]
    if name.startswith("all_active"):
        return M, M
    if name == "wide":
        return 1, SC_CAP
    return {5: (1, SC_CAP), 60: (SC_CAP + 1, SC_CAP1)}.get(s, (SC_CAP1 + 1, min(M, 1000)))


@lru_cache(maxsize=None)
def case_reference(name, dtype="float64", max_iter=1000, rows=None):
    """(codes, iterations) of the reference on a case's (first `rows`) queries, once per process."""
    X, _ = case_queries(name, dtype)
    code, iters = reference(case(name)[0], X[:rows], max_iter)
    code.setflags(write=False)
    iters.setflags(write=False)
    return code, iters


# ---------------------------------------------------------------------------------------------------
# shape sweep of the GEMMs and the epilogue: (Nq, M, d), a pruned product in which every axis value
# appears several times and the corners are kept
# ---------------------------------------------------------------------------------------------------
SWEEP_NQ = (1, 2, 63, 64, 65, 129)
SWEEP_M = (1, 2, 15, 64, 65, 130)
SWEEP_D = (1, 2, 3, 5, 17, 67, 130)
SWEEP_C = (1, 10, 70)


def sweep_shapes():
    """One combination in seven of the product, plus the corners.  A wide map (1 < d < M) whose support
    reaches d is ill conditioned (scikit-learn against itself: up to 1.7e-11 at 64 x 64 x 17, with no seed
    in 400 below 5e-13; at d = 2 a feature permutation cannot show it, but the device moved by 3.8e-11 at
    64 x 65 x 2), so with more than two query rows such a shape takes the largest M <= d instead."""
    corners = set(itertools.product((SWEEP_NQ[0], SWEEP_NQ[-1]), (SWEEP_M[0], SWEEP_M[-1]),
                                    (SWEEP_D[0], SWEEP_D[-1])))
    out = []
    for i, j, k in itertools.product(range(len(SWEEP_NQ)), range(len(SWEEP_M)), range(len(SWEEP_D))):
        nq, m, d = SWEEP_NQ[i], SWEEP_M[j], SWEEP_D[k]
        if (nq, m, d) in corners or (i + 2 * j + 3 * k) % 7 == 0:
            if 1 < d < m and nq > 2:
                m = max(v for v in SWEEP_M if v <= d)
            if (nq, m, d) not in out:
                out.append((nq, m, d))
    return out


@lru_cache(maxsize=None)
def sweep_case(nq, m, d):
    W, X = planted(d, m, min(m, d, 6), nq, 0.01, 7000 + 10007 * nq + 101 * m + d)
    W.setflags(write=False)
    X.setflags(write=False)
    return W, X
