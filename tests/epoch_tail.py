"""Cases of the epoch-tail tests (tests/test_gpu_epoch_tail_device.py, tests/test_epoch_tail_cpu.py) and of
tools/record_epoch_tail_golden.py: the counting sort behind dbgsom_accumulate, dbgsom_smooth, and one whole
dbgsom_ctx_epoch.  Everything comes from fixed seeds; the smoothing and the epoch are compared bit for bit with
tests/golden/epoch_tail_parent.npz, recorded from the library of the commit in front of the batched tail kernels
by calls both commits have (`smooth_call`, `epoch_call` below: the recorder and the test run the same code).

The formulas of accumulate.hip and smooth.hip the cases depend on are restated here (`hs_for`, `gemm_splits` in
tests/device_abi.py; the scatter kernel's LDS rule below) so that the CPU file can check every claim."""
import ctypes
import os

import numpy as np

from tests import device_abi as da

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epoch_tail_parent.npz")

# ---- the counting sort ----------------------------------------------------------------------------------------------
SORT_D = 4
# around the 64-sample rounds, the 512-sample workgroups, four of them, and hs_for's switch to 2048
SORT_N = [1, 63, 64, 65, 511, 512, 513, 2047, 2049, 300000, 300001]
# the scatter kernel's four-wavefront form keeps 4 M counters (16 M bytes) in LDS and is used while two such
# workgroups fit the 160 KB of a CU: M <= 5120; above, the one-wavefront form
SCATTER4_MAX_M = 160 * 1024 // 2 // 16
SORT_M = [1, 2, 33, 1024, SCATTER4_MAX_M, SCATTER4_MAX_M + 1]
SORT_KINDS = ["equal", "modulo", "skewed", "descending", "mixed_bad"]
SORT_SHAPES = [(N, M) for N in SORT_N for M in SORT_M]      # all five kinds at each


def sort_winners(kind, N, M, seed=0):
    """-> int64 winners; 'mixed_bad' holds -1 and M (when N >= 2: both), every other kind only [0, M)"""
    rng = np.random.default_rng(1000 * seed + 7 * N + M)
    if kind == "equal":
        return np.full(N, M // 2, dtype=np.int64)
    if kind == "modulo":
        return np.arange(N, dtype=np.int64) % M
    if kind == "skewed":                     # most rows in a few neurons, the rest thinly spread
        return np.minimum((M * rng.random(N) ** 4).astype(np.int64), M - 1)
    if kind == "descending":
        return np.sort(rng.integers(0, M, N).astype(np.int64))[::-1].copy()
    assert kind == "mixed_bad"
    w = rng.integers(0, M, N).astype(np.int64)
    bad = rng.random(N) < 0.05
    w[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, M)
    w[0] = -1
    if N > 1:
        w[N - 1] = M
    return w


def sort_rows(N, seed=0):
    """(X float32 N x SORT_D, kw, dist) of a sort case: small values, the sums are not what these tests are about"""
    rng = np.random.default_rng(seed + N)
    return rng.normal(size=(N, SORT_D)).astype(np.float32), 1.0 - rng.random(N), rng.random(N)


# ---- dbgsom_smooth --------------------------------------------------------------------------------------------------
SIGMA = 1.3
LAYOUTS = ("compact", "aligned")
# (M, d) -> split-K pieces of the product; (1030, 2): more than 1024 rows, the second trip of the strided tree
SMOOTH_CASES = {(1, 2): 1, (5, 6): 1, (17, 64): 1, (130, 66): 2, (257, 130): 4, (1030, 2): 8}
SMOOTH_NAN_CASE = (17, 64)                  # once more with a row whose every weight is zero
SMOOTH_TWICE = ((130, 66), (17, 64))        # one workspace, the larger map first


def smooth_case(M, d, nan_row=False):
    """-> (S, K, a, E, hop, W_old): sums with dead neurons (every seventh from neuron 3 on: a = K = 0, S = 0), float32
    hops on a line, cut into two disconnected parts (+inf) from M = 9 on -- every row still reaches a live neuron;
    nan_row: dead neuron 3 reaches nobody and nobody reaches it (every weight of its row is 0: W' row 3 is NaN)"""
    rng = np.random.default_rng(M * 1000 + d + (500000 if nan_row else 0))
    a = rng.integers(1, 50, M).astype(np.float64)
    dead = np.arange(M) % 7 == 3
    a[dead] = 0.0
    K = rng.uniform(0.5, 2.0, M) * a
    S = rng.normal(size=(M, d)) * K[:, None]
    S[dead] = 0.0
    E = rng.random(M) * a
    hop = np.abs(np.subtract.outer(np.arange(M), np.arange(M))).astype(np.float32)
    if M >= 9:
        part = np.arange(M) < M // 3
        hop[part[:, None] != part[None, :]] = np.inf
    if nan_row:
        assert M > 3
        hop[3, :] = np.inf
        hop[:, 3] = np.inf
        hop[3, 3] = 0.0
    W_old = rng.normal(size=(M, d))
    return S, K, a, E, hop, W_old


def smooth_key(M, d, layout, nan_row=False):
    return f"smooth_{M}_{d}_{layout}" + ("_nan" if nan_row else "")


def smooth_call(nat, case, layout, ws=None):
    """dbgsom_smooth on a fresh (or the given: (tensor, pointer, bytes)) workspace -> (W', change_total)"""
    import torch

    S, K, a, E, hop, W_old = case
    M, d = S.shape
    sums = da.dev(np.concatenate([S.reshape(-1), K, a, E]))
    hop_t, wo = da.dev(hop.astype(np.float32)), da.dev(W_old)
    wn = torch.full((M, d), float("nan"), dtype=torch.float64, device="cuda")
    chg = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    nbytes = nat.load().dbgsom_smooth_workspace_bytes(M, d)
    if ws is None:
        ws_t, ptr = da.workspace(nbytes)
    else:
        ws_t, ptr, have = ws
        assert have >= nbytes
    nat.call("dbgsom_smooth", sums.data_ptr(), M, d, hop_t.data_ptr(), SIGMA, nat.LAYOUTS[layout], wo.data_ptr(),
             wn.data_ptr(), chg.data_ptr(), ptr, nbytes, da.stream())
    torch.cuda.synchronize()
    return wn.cpu().numpy(), chg.cpu().numpy()


# ---- one epoch through the context ----------------------------------------------------------------------------------
EPOCH_SHAPE = (4096, 16, 8, 8)              # N, d, lattice rows, cols: M = 64
EPOCH_SIGMA = 1.6
EPOCH_KEYS = ("epoch_W", "epoch_errors", "epoch_activations", "epoch_change_total")


def epoch_inputs():
    N, d, rows, cols = EPOCH_SHAPE
    M = rows * cols
    rng = np.random.default_rng(4096)
    X = (rng.normal(size=(N, d)) + 3 * rng.integers(0, 5, size=(N, 1))).astype(np.float32)
    W = X[rng.choice(N, M, replace=False)].astype(np.float64)
    ii, jj = np.divmod(np.arange(M), cols)
    hop = (np.abs(ii[:, None] - ii[None]) + np.abs(jj[:, None] - jj[None])).astype(np.float64)
    gamma = float(np.var(X, axis=0).sum() ** -1)
    return X, W, hop, gamma


def epoch_call(nat):
    """one dbgsom_ctx_epoch with the filtered search -> {key: array} for EPOCH_KEYS"""
    N, d, rows, cols = EPOCH_SHAPE
    M = rows * cols
    X, W, hop, gamma = epoch_inputs()
    ctx = ctypes.c_void_p()
    nat.call("dbgsom_ctx_create", 0, ctypes.byref(ctx))
    try:
        nat.call("dbgsom_ctx_set_option", ctx, b"algorithm", nat.ALG_FILTERED)
        nat.call("dbgsom_ctx_load", ctx, X.ctypes.data, nat.F32, N, d, nat.F32)
        nat.call("dbgsom_ctx_set_topology", ctx, hop.ctypes.data, M)
        Wn, chg, E, a = np.empty((M, d)), np.empty(1), np.empty(M), np.empty(M)
        nat.call("dbgsom_ctx_epoch", ctx, W.ctypes.data, M, 0, gamma, EPOCH_SIGMA, nat.CENTRES_COMPACT, 0,
                 Wn.ctypes.data, chg.ctypes.data, E.ctypes.data, a.ctypes.data, None, None)
    finally:
        nat.call("dbgsom_ctx_destroy", ctx)
    return dict(zip(EPOCH_KEYS, (Wn, E, a, chg)))


def golden_keys():
    """every array the golden file must hold"""
    keys = []
    for (M, d) in SMOOTH_CASES:
        for layout in LAYOUTS:
            keys += [smooth_key(M, d, layout) + "_W", smooth_key(M, d, layout) + "_chg"]
    for layout in LAYOUTS:
        k = smooth_key(*SMOOTH_NAN_CASE, layout, nan_row=True)
        keys += [k + "_W", k + "_chg"]
    return keys + list(EPOCH_KEYS)
