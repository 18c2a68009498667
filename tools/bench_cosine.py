"""metric="cosine" (csrc/cosine.hip and the cosine forms of the MFMA kernels) on the MI355X against the Euclidean calls,
which run the same product loop: one JSON line per shape, also written to --out (default profiles/cosine_bench.json).

    python tools/bench_cosine.py [--steps 10] [--warmup 3] [--shapes 0,1] [--no-fit]

Shapes (float32 rows generated in HBM, prototypes = rows plus noise): 2e5 x 784 with M = 1024, 1e5 x 64 with M = 25.
HIP events on one stream, median of --steps after --warmup with [min, max]; the two sides of a pair alternate call by
call in one process on the same buffers.  The cosine side of every pair includes its two dbgsom_inv_norms launches (N
and M values) on top of the squared norms both sides are handed:
  search   dbgsom_bmu_cosine (k = 1) against dbgsom_bmu
  matrix   dbgsom_distances_cosine against dbgsom_distances, both writing the N x M matrix
  knn      dbgsom_kneighbors_cosine against dbgsom_kneighbors at k = 8 (M where M is smaller), default slab
Each pair: <name>_cosine_ms, <name>_euclid_ms, <name>_bound_ms = 1.1 * the yardstick, <name>_within_bound.
  <name>_cosine_kernel_ms     search and matrix once more with u and v already made: the kernel alone
  inv_norms_ms                the two dbgsom_inv_norms launches alone
  winners_other_than_euclid   rows whose cosine winner is not the Euclidean one
  fit_ms_<metric>             one whole SomVQ.fit (n_iter = 20, max_neurons = 100) on the device tensor (host clock)"""
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
MARGIN = 1.1


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cosine_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import SomVQ, _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_cosine.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed_pair(yard, cos):
        ty, tc = [], []
        for _ in range(a.warmup + a.steps):
            ty.append(once(yard))
            tc.append(once(cos))
        return med(ty[a.warmup:]), med(tc[a.warmup:])

    for si in (int(s) for s in a.shapes.split(",")):
        N, d, M = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        Xt = torch.randn(N, d, generator=g, device="cuda") + 3.0 * torch.randint(0, 8, (N, 1), generator=g, device="cuda")
        rng = np.random.default_rng(si)
        W = Xt[torch.from_numpy(rng.choice(N, M, replace=False)).cuda()].double().cpu().numpy()
        W += 0.05 * rng.standard_normal((M, d))
        Wt = torch.from_numpy(W).cuda()
        F32, F64 = _native.F32, _native.F64
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
        i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
        xx, ww, u, v = f64(N), f64(M), f64(N), f64(M)
        _native.call("dbgsom_row_sqnorms", Xt.data_ptr(), F32, N, d, d, xx.data_ptr(), stream)
        _native.call("dbgsom_row_sqnorms", Wt.data_ptr(), F64, M, d, d, ww.data_ptr(), stream)
        X, Wp = Xt.data_ptr(), Wt.data_ptr()

        def inv():
            _native.call("dbgsom_inv_norms", xx.data_ptr(), N, u.data_ptr(), stream)
            _native.call("dbgsom_inv_norms", ww.data_ptr(), M, v.data_ptr(), stream)

        rec = {"N": N, "d": d, "M": M, "dtype": "float32"}

        def file_pair(name, pair):
            (y, yr), (c, cr) = pair
            rec.update({f"{name}_cosine_ms": c, f"{name}_cosine_ms_min_max": cr, f"{name}_euclid_ms": y,
                        f"{name}_euclid_ms_min_max": yr, f"{name}_bound_ms": round(MARGIN * y, 4),
                        f"{name}_ratio": round(c / y, 4), f"{name}_within_bound": bool(c <= MARGIN * y)})

        idx, dist, cidx, cdist = i64(N), f64(N), i64(N), f64(N)
        file_pair("search", timed_pair(
            lambda: _native.call("dbgsom_bmu", X, F32, N, d, d, xx.data_ptr(), Wp, M, ww.data_ptr(), 1, 0, idx.data_ptr(),
                                 dist.data_ptr(), stream),
            lambda: (inv(), _native.call("dbgsom_bmu_cosine", X, F32, N, d, d, u.data_ptr(), Wp, M, v.data_ptr(), 1,
                                         cidx.data_ptr(), cdist.data_ptr(), stream))))
        rec["winners_other_than_euclid"] = int((idx != cidx).sum())
        t = [once(lambda: _native.call("dbgsom_bmu_cosine", X, F32, N, d, d, u.data_ptr(), Wp, M, v.data_ptr(), 1,
                                       cidx.data_ptr(), cdist.data_ptr(), stream)) for _ in range(a.warmup + a.steps)]
        rec["search_cosine_kernel_ms"] = med(t[a.warmup:])[0]
        rec["inv_norms_ms"] = med([once(inv) for _ in range(a.warmup + a.steps)][a.warmup:])[0]
        out = f64(N, M)
        file_pair("matrix", timed_pair(
            lambda: _native.call("dbgsom_distances", X, F32, N, d, d, xx.data_ptr(), Wp, M, ww.data_ptr(), out.data_ptr(), M,
                                 stream),
            lambda: (inv(), _native.call("dbgsom_distances_cosine", X, F32, N, d, d, u.data_ptr(), Wp, M, v.data_ptr(),
                                         out.data_ptr(), M, stream))))
        t = [once(lambda: _native.call("dbgsom_distances_cosine", X, F32, N, d, d, u.data_ptr(), Wp, M, v.data_ptr(),
                                       out.data_ptr(), M, stream)) for _ in range(a.warmup + a.steps)]
        rec["matrix_cosine_kernel_ms"] = med(t[a.warmup:])[0]
        rec["matrix_bytes"] = N * M * 8
        del out
        torch.cuda.empty_cache()
        k = min(8, M)
        nbk = int(lib.dbgsom_kneighbors_workspace_bytes(N, M, 0))
        assert nbk == int(lib.dbgsom_kneighbors_cosine_workspace_bytes(N, M, 0))
        wsk = torch.empty(nbk + 256, dtype=torch.uint8, device="cuda")
        wk = (wsk.data_ptr() + 255) // 256 * 256
        kidx, kdist = i64(N, k), f64(N, k)
        file_pair("knn", timed_pair(
            lambda: _native.call("dbgsom_kneighbors", X, F32, N, d, d, xx.data_ptr(), Wp, M, ww.data_ptr(), k, 0,
                                 kidx.data_ptr(), kdist.data_ptr(), wk, nbk, stream),
            lambda: (inv(), _native.call("dbgsom_kneighbors_cosine", X, F32, N, d, d, u.data_ptr(), Wp, M, v.data_ptr(), k, 0,
                                         kidx.data_ptr(), kdist.data_ptr(), wk, nbk, stream))))
        rec["knn_k"] = k
        rec["knn_first_is_bmu"] = bool(torch.equal(kidx[:, 0], cidx))
        del wsk, kidx, kdist
        torch.cuda.empty_cache()
        if not a.no_fit:
            for metric in ("euclidean", "cosine"):
                be = HipBackend(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    est = SomVQ(backend=be, metric=metric, random_state=0, n_iter=20, max_neurons=100).fit(Xt)
                    torch.cuda.synchronize()
                    rec[f"fit_ms_{metric}"] = round((time.perf_counter() - t0) * 1e3, 1)
                    rec[f"fit_neurons_{metric}"] = int(len(est.weights_))
                    rec[f"fit_epochs_{metric}"] = int(est.n_iter_) + 1
                except ValueError as e:
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
