"""CSR samples on the MI355X (csrc/csr.hip): the frozen-map epoch on a CSR resident, one JSON line per shape.

    python tools/bench_csr.py [--shapes tfidf256,tfidf1024,wide4096] [--steps 10] [--warmup 2] [--cpu-rows 20000]

Each line: load time, the epoch's stage split (HIP events of the context: search / sums / rest = smoothing and the
small results), the bytes of Wt the search gathers (N * stored entries per row * padded M * 8) and the rate they
arrive at, device bytes held, and the same search on the box's CPUs on the first --cpu-rows rows
(sklearn.metrics.pairwise.euclidean_distances(X_csr, W) + argmin, 16 threads) with its agreement with the device's
winners.  Data: synthetic, generated here -- about `per_row` stored entries per row, columns drawn with a
Zipf-like popularity (exponent 0.9), gamma(2, 1) values, float32; the map is M sample rows plus N(0, 0.05) noise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#         name        N        d      per_row  rows x cols
SHAPES = {"tfidf256": (200000, 50000, 100, (16, 16)),
          "tfidf1024": (200000, 50000, 100, (32, 32)),
          "wide4096": (1000000, 4096, 40, (32, 32))}


def zipf_csr(N, d, per_row, seed=0, dtype=np.float32):
    """N rows of about `per_row` distinct stored entries, column popularity ~ rank^-0.9 (ranks shuffled)."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, d + 1) ** 0.9
    cdf = np.cumsum(p / p.sum())
    cols = np.minimum(np.searchsorted(cdf, rng.random(N * per_row)), d - 1).astype(np.int64)
    key = np.unique(np.repeat(np.arange(N, dtype=np.int64), per_row) * d + rng.permutation(d)[cols])
    rows, cols = key // d, (key % d).astype(np.int32)
    indptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=N))].astype(np.int64)
    return sp.csr_matrix((rng.gamma(2.0, 1.0, key.size).astype(dtype), cols, indptr), shape=(N, d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tfidf256,tfidf1024,wide4096")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-rows", type=int, default=20000)
    a = ap.parse_args()
    import bench
    from dbgsom_amd import _native
    from dbgsom_amd.backend import RESIDENT, HipBackend

    for name in a.shapes.split(","):
        N, d, per_row, (rows, cols) = SHAPES[name]
        M = rows * cols
        X = zipf_csr(N, d, per_row)
        rng = np.random.default_rng(1)
        W = X[np.sort(rng.choice(N, M, replace=False))].toarray().astype(np.float64) + rng.normal(0, 0.05, (M, d))
        hop = bench.lattice_hops(rows, cols)
        hip = HipBackend(0)
        hip.csr_densify_below = 0
        hip._set("timing", 1)
        t0 = time.perf_counter()
        hip.load(X)
        t_load = time.perf_counter() - t0
        assert hip.resident_csr
        hip.set_weights(W)
        hip.phase_log = []
        wall = []
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            res = hip.epoch(RESIDENT, hop, 2.0, 1e-3, "compact", keep_on_device=True, frozen=True)
            wall.append(time.perf_counter() - t0)
        ph = np.array(hip.phase_log[a.warmup:])[:, :3]        # [search, sums, smoothing + results] ms
        search, sums, rest = (float(v) for v in np.median(ph, axis=0))
        epoch_ms = float(np.median(wall[a.warmup:]) * 1e3)
        ldwt = _native.load().dbgsom_csr_wt_ld(M)
        gathered = X.nnz * ldwt * 8
        dist, win = hip.bmu(RESIDENT, 1)
        dev_bytes = hip._get("device_bytes")
        hip.release()
        # the same search on the CPUs
        from sklearn.metrics.pairwise import euclidean_distances
        from threadpoolctl import threadpool_limits

        nc = min(N, a.cpu_rows)
        with threadpool_limits(limits=16):
            t0 = time.perf_counter()
            cpu_win = euclidean_distances(X[:nc], W).argmin(axis=1)
            t_cpu = time.perf_counter() - t0
        line = {"shape": name, "N": N, "d": d, "M": M, "nnz": int(X.nnz), "stored_per_row": round(X.nnz / N, 2),
                "dtype": "float32", "load_s": round(t_load, 3), "epoch_ms": round(epoch_ms, 3),
                "search_ms": round(search, 3), "sums_ms": round(sums, 3), "rest_ms": round(rest, 3),
                "samples_per_s": round(N / (epoch_ms * 1e-3)),
                "wt_bytes": int(d * ldwt * 8), "wt_gathered_bytes": int(gathered),
                "wt_gathered_bytes_per_s": round(gathered / (search * 1e-3)),
                "search_gflops": round(2.0 * X.nnz * M / (search * 1e-3) / 1e9, 1),
                "device_bytes": int(dev_bytes), "dense_f32_bytes": int(N) * d * 4,
                "hit_neurons": int(np.count_nonzero(res.activations)),
                "cpu_rows": nc, "cpu_search_s": round(t_cpu, 3), "cpu_samples_per_s": round(nc / t_cpu),
                "cpu_winner_agreement": float(np.mean(cpu_win == win[:nc]))}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
