"""metric="manhattan" (csrc/manhattan.hip) on the MI355X against the parent's masked search, which issues the same two
vector instructions per entry plus a scalar NaN branch: one JSON line per shape, also written to --out (default
profiles/manhattan_bench.json).

    python tools/bench_manhattan.py [--steps 10] [--warmup 3] [--shapes 0,1] [--no-fit]

Shapes (float32 rows generated in HBM without NaN, prototypes = rows plus noise): 2e5 x 784 with M = 1024, 1e5 x 64 with
M = 25.  Each line, HIP events on one stream, median of --steps after --warmup with [min, max], every figure of a line
from the same process on the same GPU:
  l1_ms         dbgsom_bmu_manhattan, k = 1 (transposition of the prototypes and widening of the rows included)
  masked_ms     dbgsom_bmu_masked on the same buffers: the yardstick; bound_ms = 1.1 * masked_ms,
                within_bound = l1_ms <= bound_ms
  euclid_ms     dbgsom_bmu (the all-pairs MFMA search) on the same buffers, for scale
  matrix_ms     dbgsom_distances_manhattan writing the N x M matrix; fill_ms: a plain device write of as many bytes
  knn_ms        dbgsom_kneighbors_manhattan at k = 8 (M where M is smaller), default slab
  pairs_per_s   N M d / l1_ms; vector_peak_share: two float64 instruction lanes per (pair, feature) against the
                78.6 TFLOP/s float64 vector peak (which counts a fused multiply-add as two)
  fit_ms        one whole SomVQ.fit (n_iter = 20, max_neurons = 100) on the device tensor under each metric (host clock);
                fit_error_<metric>: the fit refused (rows this wide under the L1 metric: DESIGN 4j)"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(200_000, 784, 1024), (100_000, 64, 25)]
VECTOR_F64_PEAK = 78.6e12


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manhattan_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import SomVQ, _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_manhattan.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def timed(fn):
        t = []
        for _ in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return med(t[a.warmup:])

    for si in (int(s) for s in a.shapes.split(",")):
        N, d, M = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        Xt = torch.randn(N, d, generator=g, device="cuda") + 3.0 * torch.randint(0, 8, (N, 1), generator=g, device="cuda")
        rng = np.random.default_rng(si)
        W = Xt[torch.from_numpy(rng.choice(N, M, replace=False)).cuda()].double().cpu().numpy()
        W += 0.05 * rng.standard_normal((M, d))
        Wt = torch.from_numpy(W).cuda()
        idx = torch.empty(N, dtype=torch.int64, device="cuda")
        dist = torch.empty(N, dtype=torch.float64, device="cuda")
        F32, F64 = _native.F32, _native.F64

        def ws_of(nbytes):
            return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device="cuda"), int(nbytes)

        ws, nb = ws_of(lib.dbgsom_bmu_manhattan_workspace_bytes(F32, N, d, M))
        l1 = timed(lambda: _native.call("dbgsom_bmu_manhattan", Xt.data_ptr(), F32, N, d, d, Wt.data_ptr(), M, d, 1,
                                        idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), nb, stream))
        l1_idx = idx.clone()
        wsm, nbm = ws_of(lib.dbgsom_bmu_masked_workspace_bytes(F32, N, d, M))
        masked = timed(lambda: _native.call("dbgsom_bmu_masked", Xt.data_ptr(), F32, N, d, d, Wt.data_ptr(), M, d, 1,
                                            idx.data_ptr(), dist.data_ptr(), wsm.data_ptr(), nbm, stream))
        del wsm
        xx = torch.empty(N, dtype=torch.float64, device="cuda")
        ww = torch.empty(M, dtype=torch.float64, device="cuda")
        _native.call("dbgsom_row_sqnorms", Xt.data_ptr(), F32, N, d, d, xx.data_ptr(), stream)
        _native.call("dbgsom_row_sqnorms", Wt.data_ptr(), F64, M, d, d, ww.data_ptr(), stream)
        euclid = timed(lambda: _native.call("dbgsom_bmu", Xt.data_ptr(), F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                                            ww.data_ptr(), 1, 0, idx.data_ptr(), dist.data_ptr(), stream))
        differ = int((idx != l1_idx).sum())
        out = torch.empty((N, M), dtype=torch.float64, device="cuda")
        matrix = timed(lambda: _native.call("dbgsom_distances_manhattan", Xt.data_ptr(), F32, N, d, d, Wt.data_ptr(), M, d,
                                            out.data_ptr(), M, ws.data_ptr(), nb, stream))
        fill = timed(lambda: out.fill_(1.0))
        del out, ws
        torch.cuda.empty_cache()
        k = min(8, M)
        wsk, nbk = ws_of(lib.dbgsom_kneighbors_manhattan_workspace_bytes(F32, N, d, M, 0))
        wk = (wsk.data_ptr() + 255) // 256 * 256
        kidx = torch.empty((N, k), dtype=torch.int64, device="cuda")
        kdist = torch.empty((N, k), dtype=torch.float64, device="cuda")
        knn = timed(lambda: _native.call("dbgsom_kneighbors_manhattan", Xt.data_ptr(), F32, N, d, d, Wt.data_ptr(), M, d, k,
                                         0, kidx.data_ptr(), kdist.data_ptr(), wk, nbk, stream))
        same_first = bool(torch.equal(kidx[:, 0], l1_idx))
        del wsk, kidx, kdist
        torch.cuda.empty_cache()
        bound = round(1.1 * masked[0], 4)
        pairs = float(N) * M * d
        rec = {"N": N, "d": d, "M": M, "dtype": "float32", "l1_ms": l1[0], "l1_ms_min_max": l1[1],
               "masked_ms": masked[0], "masked_ms_min_max": masked[1], "bound_ms": bound,
               "within_bound": bool(l1[0] <= bound), "euclid_ms": euclid[0], "euclid_ms_min_max": euclid[1],
               "winners_other_than_euclid": differ, "matrix_ms": matrix[0], "matrix_ms_min_max": matrix[1],
               "fill_ms": fill[0], "matrix_bytes": N * M * 8, "knn_k": k, "knn_ms": knn[0], "knn_ms_min_max": knn[1],
               "knn_first_is_bmu": same_first, "pairs_per_s": round(pairs / (l1[0] * 1e-3), 1),
               "vector_peak_share": round(2.0 * pairs / (l1[0] * 1e-3) / (VECTOR_F64_PEAK / 2.0), 4)}
        if not a.no_fit:
            for metric in ("euclidean", "manhattan"):
                be = HipBackend(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    est = SomVQ(backend=be, metric=metric, random_state=0, n_iter=20, max_neurons=100).fit(Xt)
                    torch.cuda.synchronize()
                    rec[f"fit_ms_{metric}"] = round((time.perf_counter() - t0) * 1e3, 1)
                    rec[f"fit_neurons_{metric}"] = int(len(est.weights_))
                    rec[f"fit_epochs_{metric}"] = int(est.n_iter_) + 1
                except ValueError as e:   # (wide rows under the L1 metric: the sample kernel underflows)
                    rec[f"fit_error_{metric}"] = str(e)[:120]
                be.release()
        rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del Xt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
