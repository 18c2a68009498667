"""Sparse coding throughput on the MI355X (csrc/sparse_code.hip): one JSON line per shape.

    python tools/bench_sparse_code.py [--shapes c2,c4] [--transform-rows N]

Each line: ms and samples/s of predict_proba (all query rows, the code never leaves the device) and of
transform (the first --transform-rows rows: the N x M code is copied back), the device counters of the
predict_proba call; the stage split of a second, timed predict_proba call (HIP events: Gram, Cov GEMM,
LARS, the two overflow passes), the Cov GEMM against the f64 MFMA peak and the LARS stage against its
modelled G-row bytes; and scikit-learn's SparseCoder on a 2000-row subset (n_jobs=16): its samples/s
and the max |dcode| against the device.  Data: bench.py's generator (blobs, float32); the map is M
sample rows plus N(0, 0.1) noise, P random class frequencies over 10 classes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c2": (60000, 784, 506), "c4": (1000000, 784, 1024)}
F64_MFMA_PEAK = 78.6e12        # FLOP/s (MI355X_MICROARCH.md)
INFINITY_CACHE_BW = 8.6e12     # bytes/s
GATES = {"c2": ("predict_proba_s", 0.15), "c4": ("predict_proba_samples_per_s", 5e5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c4")
    ap.add_argument("--transform-rows", type=int, default=100000)
    ap.add_argument("--sklearn-rows", type=int, default=2000)
    a = ap.parse_args()
    import ctypes

    import bench
    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    hip = HipBackend(0)
    for name in a.shapes.split(","):
        N, d, M = SHAPES[name]
        X = bench.make_shard_numpy(N, d, 0)
        rng = np.random.default_rng(1)
        W = X[rng.choice(N, M, replace=False)].astype(np.float64) + rng.normal(0, 0.1, (M, d))
        P = rng.random((M, 10))
        P /= P.sum(axis=1, keepdims=True)
        hip.sparse_code(W, X[:min(N, hip.sc_chunk_rows)], P=P)  # warm-up: allocations of a full chunk
        t0 = time.perf_counter()
        hip.sparse_code(W, X, P=P)
        t_pp = time.perf_counter() - t0
        counts = dict(hip.sparse_code_counts)
        # stage split: the same call again with HIP events around the stages (blocking per chunk)
        lib = _native.load()
        lib.dbgsom_sparse_code_timing(1)
        t0 = time.perf_counter()
        hip.sparse_code(W, X, P=P)
        t_timed = time.perf_counter() - t0
        ms = (ctypes.c_double * 5)()
        _native.call("dbgsom_sparse_code_stage_ms", ms)
        lib.dbgsom_sparse_code_timing(0)
        ms = [float(v) for v in ms]
        g_bytes = counts["g_rows"] * M * 8
        split = {"gram_ms": round(ms[0], 3), "cov_gemm_ms": round(ms[1], 3), "lars_ms": round(ms[2], 3),
                 "overflow1_ms": round(ms[3], 3), "overflow2_ms": round(ms[4], 3),
                 "other_ms": round(t_timed * 1e3 - sum(ms), 3), "timed_call_s": round(t_timed, 4),
                 "cov_gemm_frac_f64_peak": round(2.0 * N * M * d / (ms[1] * 1e-3) / F64_MFMA_PEAK, 4),
                 "lars_model_g_row_bytes": g_bytes,
                 "lars_g_row_bytes_per_s": round(g_bytes / ((ms[2] + ms[3] + ms[4]) * 1e-3)),
                 "lars_model_ms_at_infinity_cache_bw": round(g_bytes / INFINITY_CACHE_BW * 1e3, 3)}
        nt = min(N, a.transform_rows)
        t0 = time.perf_counter()
        code = hip.sparse_code(W, X[:nt])
        t_tr = time.perf_counter() - t0
        from sklearn.decomposition import SparseCoder
        from sklearn.preprocessing import normalize

        ns = min(a.sklearn_rows, N)
        coder = SparseCoder(dictionary=normalize(W), positive_code=True, transform_alpha=0,
                            transform_algorithm="lasso_lars", n_jobs=16)
        t0 = time.perf_counter()
        ref = coder.transform(normalize(X[:ns]))
        t_sk = time.perf_counter() - t0
        line = {"shape": name, "N": N, "d": d, "M": M,
                "predict_proba_s": round(t_pp, 4), "predict_proba_samples_per_s": round(N / t_pp),
                "transform_rows": nt, "transform_s": round(t_tr, 4), "transform_samples_per_s": round(nt / t_tr),
                "counts": counts, "stages": split, "mean_iterations": counts["iterations"] / max(counts["samples"], 1),
                "sklearn_rows": ns, "sklearn_samples_per_s": round(ns / t_sk),
                "max_abs_dcode": float(np.abs(code[:ns] - ref).max())}
        key, bound = GATES[name]
        line["gate"] = {key: bound, "met": bool(line[key] >= bound if key.endswith("_per_s") else line[key] <= bound)}
        print(json.dumps(line), flush=True)
    hip.release()


if __name__ == "__main__":
    main()
