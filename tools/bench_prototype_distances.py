"""The distance-matrix kernel (csrc/distances.hip) against the all-pairs search it is derived from, on the MI355X: one
JSON line per shape, also written to --out (default profiles/prototype_distances_bench.json).

    python tools/bench_prototype_distances.py [--steps 10] [--warmup 3] [--host-steps 3] [--shapes 0,1,2]

Shapes (float32 rows generated in HBM, prototypes = rows plus noise): 1e6 x 784 with M = 1024, 1e6 x 784 with M = 100
(a fitted map's usual size), 1e5 x 64 with M = 25.  Each line, HIP events on one stream, median of --steps after
--warmup with [min, max], every figure of a line from the same process on the same GPU:
  distances_ms      dbgsom_distances on the rows in HBM (norms made beforehand, as for the search)
  search_ms         dbgsom_bmu, k = 1, all pairs, on the same buffers
  write_ms          a plain device write of N * M * 8 bytes (fill_ of the result tensor)
  bound_ms          1.1 * (search_ms + write_ms): a kernel with no overlap between products and stores, plus the
                    spread between boxes; within_bound = distances_ms <= bound_ms
  host_ms           the whole HipBackend.distances call on the same rows as a host array (host clock, --host-steps),
                    device_in_host_ms the kernels inside it (distances_ms and the norms, per chunk), and the rates of
                    a pageable copy of X up and of the result down on their own (upload_bytes_per_s,
                    download_bytes_per_s) next to the rate both reach inside the call (transfer_bytes_per_s: the
                    call's traffic counters over host_ms - device_in_host_ms)
  max_abs_diff_sklearn   largest |D - euclidean_distances(X, W)| over the first 2000 rows"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 784, 1024), (1_000_000, 784, 100), (100_000, 64, 25)]


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prototype_distances_bench.json"))
    a = ap.parse_args()
    import torch
    from sklearn.metrics import euclidean_distances

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_prototype_distances.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    be = HipBackend(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []
    for si in (int(s) for s in a.shapes.split(",")):
        N, d, M = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        Xt = torch.randn(N, d, generator=g, device="cuda") + 3.0 * torch.randint(0, 8, (N, 1), generator=g, device="cuda")
        rng = np.random.default_rng(si)
        W = Xt[torch.from_numpy(rng.choice(N, M, replace=False)).cuda()].double().cpu().numpy()
        W += 0.05 * rng.standard_normal((M, d))
        Wt = torch.from_numpy(W).cuda()
        xx = torch.empty(N, dtype=torch.float64, device="cuda")
        ww = torch.empty(M, dtype=torch.float64, device="cuda")
        out = torch.empty((N, M), dtype=torch.float64, device="cuda")
        idx = torch.empty(N, dtype=torch.int64, device="cuda")
        dist = torch.empty(N, dtype=torch.float64, device="cuda")
        _native.call("dbgsom_row_sqnorms", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), stream)
        _native.call("dbgsom_row_sqnorms", Wt.data_ptr(), _native.F64, M, d, d, ww.data_ptr(), stream)

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

        d_ms, d_mm = timed(lambda: _native.call("dbgsom_distances", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(),
                                                Wt.data_ptr(), M, ww.data_ptr(), out.data_ptr(), M, stream))
        s_ms, s_mm = timed(lambda: _native.call("dbgsom_bmu", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(),
                                                Wt.data_ptr(), M, ww.data_ptr(), 1, 0, idx.data_ptr(), dist.data_ptr(),
                                                stream))
        consistent = bool(torch.equal(out.min(dim=1).values, dist))
        head = out[:2000].cpu().numpy()
        w_ms, w_mm = timed(lambda: out.fill_(1.0))
        n_ms, _ = timed(lambda: _native.call("dbgsom_row_sqnorms", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(),
                                             stream))
        bound = 1.1 * (s_ms + w_ms)
        Xh = Xt.cpu().numpy()
        diff = float(np.abs(head - euclidean_distances(Xh[:2000].astype(np.float64), W)).max())
        del out, idx, dist
        torch.cuda.empty_cache()

        before = be.sample_traffic()
        res = be.distances(W, Xh)
        after = be.sample_traffic()
        up, down = (after[k] - before[k] for k in ("x_upload_bytes", "x_download_bytes"))
        equal_head = bool(np.array_equal(res[:2000], head))
        t = []
        for _ in range(a.host_steps):
            t0 = time.perf_counter()
            be.distances(W, Xh)
            t.append((time.perf_counter() - t0) * 1e3)
        h_ms, h_mm = med(t)
        dev_in_host = d_ms + n_ms
        t0 = time.perf_counter()
        Xc = torch.from_numpy(Xh).cuda()
        torch.cuda.synchronize()
        up_s = time.perf_counter() - t0
        rt = torch.empty((min(N, 200_000), M), dtype=torch.float64, device="cuda").fill_(1.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.cpu()
        down_s = time.perf_counter() - t0
        rec = {"N": N, "d": d, "M": M, "dtype": "float32", "distances_ms": d_ms, "distances_ms_min_max": d_mm,
               "search_ms": s_ms, "search_ms_min_max": s_mm, "write_ms": w_ms, "write_ms_min_max": w_mm,
               "bound_ms": round(bound, 4), "within_bound": bool(d_ms <= bound),
               "row_minima_equal_search": consistent, "result_bytes": N * M * 8,
               "store_bytes_per_s": round(N * M * 8 / (d_ms * 1e-3)),
               "host_ms": h_ms, "host_ms_min_max": h_mm, "device_in_host_ms": round(dev_in_host, 4),
               "x_upload_bytes": up, "x_download_bytes": down,
               "transfer_bytes_per_s": round((up + down) / max((h_ms - dev_in_host) * 1e-3, 1e-9)),
               "upload_bytes_per_s": round(Xh.nbytes / up_s), "download_bytes_per_s": round(rt.numel() * 8 / down_s),
               "host_equals_device_head": equal_head, "max_abs_diff_sklearn": diff,
               "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del Xc, rt, res, Xt, Xh
        torch.cuda.empty_cache()
    be.release()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
