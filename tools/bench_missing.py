"""Queries on rows with missing entries on the MI355X (csrc/masked.hip): one JSON line per shape and share of
missing cells, also appended to --out (default profiles/missing_bench.json).

    python tools/bench_missing.py [--shapes wide,narrow] [--fracs 0.01,0.1,0.5] [--steps 10] [--warmup 2]

Each line:
  device_ms        dbgsom_bmu_masked on the whole batch in HBM, HIP events around the call on its stream: the
                   transposition of W, the pass that counts the observed entries (and widens float32 rows) and the
                   search; median of --steps
  matrix_ms        dbgsom_distances_masked writing the N x M matrix, and knn_ms: dbgsom_kneighbors_masked with k = 8 (or M)
                   at the default slab; HIP events as device_ms, median of --steps
  call_ms          HipBackend.bmu_masked from host arrays (chunked upload, search, download), host clock around the
                   blocking call; median of --steps
  rows_per_s       N / device_ms, and call_rows_per_s = N / call_ms
  pairs_per_s      observed cells x M (one float64 subtract and one fma each) / device_ms, and its share of the vector
                   float64 peak: 78.6 TFLOP/s counts an fma as two, so 39.3e12 instruction lanes/s, two per pair
  wt_read_bytes    bytes of the transposed prototypes the search reads (workgroups x d x padded M x 8) and their rate
  exact_*          for scale: the all-pairs query as it exists (dbgsom_bmu on the device; HipBackend(algorithm="exact")
                   .bmu from the host) on the same rows with NaN set to 0
  oracle_*         NumPy, direct form, on the first --oracle-rows rows: largest relative distance difference and the
                   number of differing winners
Data: seeded; 8 centres 3 N(0, 1), rows and prototypes = a centre + N(0, 1), float32 rows, cells punched out with
probability frac (one random cell per row kept)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"wide": (200000, 784, 1024), "narrow": (200000, 64, 256)}
PEAK_F64_VECTOR_FLOPS = 78.6e12
ROWS_PER_WORKGROUP = 16   # csrc/direct_rows.h: MR (batches of 8192 rows and more)


def make(N, d, M, frac, seed=0):
    rng = np.random.default_rng(seed)
    C = 3.0 * rng.standard_normal((8, d))
    W = C[rng.integers(0, 8, M)] + rng.standard_normal((M, d))
    X = (C[rng.integers(0, 8, N)] + rng.standard_normal((N, d), dtype=np.float32)).astype(np.float32)
    holes = rng.random((N, d), dtype=np.float32) < frac
    holes[np.arange(N), rng.integers(0, d, N)] = False
    X[holes] = np.nan
    return X, W


def oracle(X, W, step=16):
    X64 = X.astype(np.float64)
    obs = ~np.isnan(X64)
    d = X.shape[1]
    out = np.empty((X.shape[0], W.shape[0]))
    for lo in range(0, X.shape[0], step):
        diff = np.where(obs[lo:lo + step, None, :], X64[lo:lo + step, None, :] - W[None], 0.0)
        out[lo:lo + step] = np.sqrt((diff ** 2).sum(axis=2) * (d / obs[lo:lo + step].sum(axis=1))[:, None])
    return out


def median_ms(fn, steps, warmup):
    t = [fn() for _ in range(warmup + steps)][warmup:]
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="wide,narrow")
    ap.add_argument("--fracs", default="0.01,0.1,0.5")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-rows", type=int, default=2000)
    ap.add_argument("--rows", type=int, default=0, help="override N (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "missing_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_missing.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    hip = HipBackend(0)
    exact = HipBackend(0, algorithm="exact")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    def walled(fn):
        def run():
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        return run

    lines = []
    for name in a.shapes.split(","):
        N, d, M = SHAPES[name]
        N = a.rows or N
        for frac in (float(f) for f in a.fracs.split(",")):
            X, W = make(N, d, M, frac)
            observed = int((~np.isnan(X)).sum())
            Xt, Wt = torch.from_numpy(X).cuda(), torch.from_numpy(W).cuda()
            idx = torch.empty((N, 1), dtype=torch.int64, device="cuda")
            dist = torch.empty((N, 1), dtype=torch.float64, device="cuda")
            nbytes = lib.dbgsom_bmu_masked_workspace_bytes(_native.F32, N, d, M)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            dev = median_ms(timed(lambda: _native.call(
                "dbgsom_bmu_masked", Xt.data_ptr(), _native.F32, N, d, d, Wt.data_ptr(), M, d, 1, idx.data_ptr(),
                dist.data_ptr(), ws.data_ptr(), nbytes, stream)), a.steps, a.warmup)
            dev_idx, dev_dist = idx.cpu().numpy().reshape(-1), dist.cpu().numpy().reshape(-1)
            # the siblings that store every pair: the N x M matrix, and the k nearest through slabs of it
            out = torch.empty((N, M), dtype=torch.float64, device="cuda")
            matrix = median_ms(timed(lambda: _native.call(
                "dbgsom_distances_masked", Xt.data_ptr(), _native.F32, N, d, d, Wt.data_ptr(), M, d, out.data_ptr(), M,
                ws.data_ptr(), nbytes, stream)), a.steps, a.warmup)
            del out
            kk = min(8, M)
            kbytes = lib.dbgsom_kneighbors_masked_workspace_bytes(_native.F32, N, d, M, 0)
            kws = torch.empty(kbytes, dtype=torch.uint8, device="cuda")
            kidx = torch.empty((N, kk), dtype=torch.int64, device="cuda")
            kdist = torch.empty((N, kk), dtype=torch.float64, device="cuda")
            knn = median_ms(timed(lambda: _native.call(
                "dbgsom_kneighbors_masked", Xt.data_ptr(), _native.F32, N, d, d, Wt.data_ptr(), M, d, kk, 0,
                kidx.data_ptr(), kdist.data_ptr(), kws.data_ptr(), kbytes, stream)), a.steps, a.warmup)
            del kws, kidx, kdist
            call = median_ms(walled(lambda: hip.bmu_masked(W, 1, X)), a.steps, a.warmup)
            # for scale: the all-pairs search on the zero-filled rows
            X0 = np.nan_to_num(X, nan=0.0)
            X0t = torch.from_numpy(X0).cuda()
            xx = torch.empty(N, dtype=torch.float64, device="cuda")
            ww = torch.empty(M, dtype=torch.float64, device="cuda")
            _native.call("dbgsom_row_sqnorms", X0t.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), stream)
            _native.call("dbgsom_row_sqnorms", Wt.data_ptr(), _native.F64, M, d, d, ww.data_ptr(), stream)
            ex_dev = median_ms(timed(lambda: _native.call(
                "dbgsom_bmu", X0t.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M, ww.data_ptr(), 1, 0,
                idx.data_ptr(), dist.data_ptr(), stream)), a.steps, a.warmup)
            ex_call = median_ms(walled(lambda: exact.bmu(W, 1, X=X0)), a.steps, a.warmup)
            del Xt, X0t, ws
            # the oracle on the first rows
            n_or = min(N, a.oracle_rows)
            D = oracle(X[:n_or], W)
            want_idx = D.argmin(axis=1)
            want_dist = D[np.arange(n_or), want_idx]
            rel = float(np.max(np.abs(dev_dist[:n_or] - want_dist) / np.where(want_dist > 0, want_dist, 1.0)))
            ldwt = lib.dbgsom_csr_wt_ld(M)
            groups = -(-N // ROWS_PER_WORKGROUP)
            wt_read = groups * d * ldwt * 8
            pairs = observed * M
            line = {"shape": name, "N": N, "d": d, "M": M, "dtype": "float32", "missing": frac,
                    "observed_cells": observed,
                    "device_ms": round(dev[0], 3), "device_ms_min_max": [round(dev[1], 3), round(dev[2], 3)],
                    "matrix_ms": round(matrix[0], 3), "matrix_ms_min_max": [round(matrix[1], 3), round(matrix[2], 3)],
                    "knn_ms": round(knn[0], 3), "knn_ms_min_max": [round(knn[1], 3), round(knn[2], 3)], "knn_k": kk,
                    "call_ms": round(call[0], 3), "call_ms_min_max": [round(call[1], 3), round(call[2], 3)],
                    "rows_per_s": round(N / (dev[0] * 1e-3)), "call_rows_per_s": round(N / (call[0] * 1e-3)),
                    "pairs_per_s": round(pairs / (dev[0] * 1e-3)),
                    "share_of_f64_vector_peak": round(pairs * 4.0 / (dev[0] * 1e-3) / PEAK_F64_VECTOR_FLOPS, 4),
                    "wt_read_bytes": int(wt_read), "wt_read_bytes_per_s": round(wt_read / (dev[0] * 1e-3)),
                    "exact_device_ms": round(ex_dev[0], 3), "exact_call_ms": round(ex_call[0], 3),
                    "oracle_rows": n_or, "oracle_max_rel_dist_diff": rel,
                    "oracle_winners_differing": int(np.count_nonzero(dev_idx[:n_or] != want_idx)),
                    "steps": a.steps, "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
