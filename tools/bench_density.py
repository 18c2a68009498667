"""The rows within a radius of every prototype (csrc/density.hip) against the neighbour search at k = 1 that it is built
beside, and against what a user did before it, on the MI355X: one JSON line per shape and number of radii, also written
to --out (default profiles/density_bench.json).

    python tools/bench_density.py [--steps 10] [--warmup 3] [--shapes 0,1,2] [--radii 1,8,32] [--no-host] [--no-torch]

Shapes of tools/bench_exemplars.py (float32 rows generated in HBM, prototypes = rows plus noise): 1e6 x 784 with
M = 1024 and M = 100, 1e5 x 64 with M = 25.  The radii are quantiles (1 % .. 50 %) of the distances of the first 4096
rows.  HIP events on one stream, median of --steps after --warmup with [min, max]; the two sides of a comparison
alternate inside one loop, every figure of a line from the same process on the same GPU.  The count and the selection
at k = 1 read the slab once from cache behind the same product kernel, so the yardstick of the device time is
dbgsom_kneighbors at k = 1, existing code; the margin of 10 % is the verdict of n_radii = 1, and a line that misses it
says so and names the kernel that costs it.  At 8 and 32 radii the ratio is reported without a bound:
  T_kn_ms       dbgsom_kneighbors at k = 1 on the same buffers, default slab (the yardstick)
  T_rc_ms       dbgsom_range_counts at n_radii; ratio = T_rc / T_kn; within_margin (n_radii = 1 only): ratio <= 1.1
  T_rows_ms     dbgsom_topk_rows at k = 1 on one resident slab of slab_rows x M squared values
  T_fold_ms     dbgsom_range_count_cols on the same slab; fold_over_rows = T_fold / T_rows
  missed_by     for a line outside the margin: the kernel whose time on a slab exceeds the row selection's
  call_ms       the whole HipBackend.range_counts call on the device tensor (host clock), peak_bytes its torch peak plus
                the workspace of dbgsom_range_counts
  torch_ms      (backend.distances(W, X) <= rho).sum(0) per radius in torch (host clock), torch_peak_bytes its torch
                peak; same_counts: equal counts
  host_ms       the call on the same rows as a host array, with its PCIe bytes (x_upload_bytes, x_download_bytes)"""
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
MARGIN = 1.1


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--radii", default="1,8,32")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend, squared_thresholds

    if not torch.cuda.is_available():
        raise SystemExit("bench_density.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    be = HipBackend(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def timed(*fns):
        """the sides alternating: -> (median, [min, max]) of each"""
        ts = [[] for _ in fns]
        for _ in range(a.warmup + a.steps):
            for fn, t in zip(fns, ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
        return [med(t[a.warmup:]) for t in ts]

    def clocked(fn, steps=3):
        t = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return med(t)

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
        _native.call("dbgsom_row_sqnorms", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), stream)
        _native.call("dbgsom_row_sqnorms", Wt.data_ptr(), _native.F64, M, d, d, ww.data_ptr(), stream)
        ldr = M + M % 2
        ws_bytes = lib.dbgsom_range_counts_workspace_bytes(N, M, 0)      # (that of dbgsom_kneighbors)
        rows = min(N, ws_bytes // (ldr * 8))
        slabs = -(-N // rows)
        sample = be.distances(W, Xt[:4096]).cpu().numpy()
        Xh = None if a.no_host else Xt.cpu().numpy()
        for n in (int(s) for s in a.radii.split(",")):
            radii = np.quantile(sample, np.linspace(0.01, 0.5, n))
            thr = squared_thresholds(radii)
            thr_t = torch.from_numpy(thr).cuda()
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            idx = torch.empty(N, dtype=torch.int64, device="cuda")
            dist = torch.empty(N, dtype=torch.float64, device="cuda")
            counts = torch.empty((M, n), dtype=torch.int64, device="cuda")

            def kn():
                _native.call("dbgsom_kneighbors", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                             ww.data_ptr(), 1, 0, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, stream)

            def rc():
                _native.call("dbgsom_range_counts", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                             ww.data_ptr(), thr_t.data_ptr(), n, 0, counts.data_ptr(), ws.data_ptr(), ws_bytes, stream)

            (tk, tk_mm), (tc, tc_mm) = timed(kn, rc)
            # one resident slab: what the product kernel left in the workspace for the last slab's rows
            n_last = N - (slabs - 1) * rows
            R = ws.view(torch.float64)[: rows * ldr].view(rows, ldr)
            if n_last < rows:     # fill the slab with whole rows of squared values
                R[n_last:] = R[:n_last].repeat(-(-rows // n_last), 1)[: rows - n_last]
            state = torch.zeros((M, n), dtype=torch.int64, device="cuda")

            def sel_rows():
                _native.call("dbgsom_topk_rows", R.data_ptr(), rows, M, ldr, 1, idx.data_ptr(), dist.data_ptr(), stream)

            def fold():
                _native.call("dbgsom_range_count_cols", R.data_ptr(), rows, M, ldr, thr_t.data_ptr(), n, state.data_ptr(),
                             stream)

            (tr, tr_mm), (tf, tf_mm) = timed(sel_rows, fold)
            rec = {"N": N, "d": d, "M": M, "n_radii": n, "dtype": "float32", "slab_rows": rows, "slabs": slabs,
                   "T_kn_ms": tk, "T_kn_ms_min_max": tk_mm, "T_rc_ms": tc, "T_rc_ms_min_max": tc_mm,
                   "ratio": round(tc / tk, 3), "T_rows_ms": tr, "T_rows_ms_min_max": tr_mm, "T_fold_ms": tf,
                   "T_fold_ms_min_max": tf_mm, "fold_over_rows": round(tf / tr, 3), "slab_bytes": int(rows * ldr * 8)}
            if n == 1:
                rec.update({"margin": MARGIN, "within_margin": bool(tc <= MARGIN * tk)})
                if not rec["within_margin"]:
                    rec["missed_by"] = ["range_count_cols_kernel<1>: %.4f ms per slab against %.4f ms of topk_rows_kernel<1>"
                                        % (tf, tr)]
            del ws, R, idx, dist, state
            torch.cuda.empty_cache()

            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            cc = be.range_counts(W, thr, Xt)
            torch.cuda.synchronize()
            rec["peak_bytes"] = int(torch.cuda.max_memory_allocated() - base + ws_bytes)
            rec["device_call_equals_raw"] = bool(torch.equal(cc, counts))
            rec["call_ms"], rec["call_ms_min_max"] = clocked(lambda: be.range_counts(W, thr, Xt))
            if not a.no_torch:
                def torch_route():
                    D = be.distances(W, Xt)
                    return torch.stack([(D <= float(r)).sum(0) for r in radii], dim=1)

                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                tc_ = torch_route()
                torch.cuda.synchronize()
                rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
                rec["same_counts"] = bool(torch.equal(tc_, cc))
                del tc_
                torch.cuda.empty_cache()
                rec["torch_ms"], rec["torch_ms_min_max"] = clocked(torch_route)
                torch.cuda.empty_cache()
            rec["matrix_bytes"] = N * M * 8
            if Xh is not None:
                before = be.sample_traffic()
                hc = be.range_counts(W, thr, Xh)
                after = be.sample_traffic()
                rec.update({"x_upload_bytes": after["x_upload_bytes"] - before["x_upload_bytes"],
                            "x_download_bytes": after["x_download_bytes"] - before["x_download_bytes"],
                            "host_equals_device": bool(np.array_equal(hc, cc.cpu().numpy()))})
                rec["host_ms"], rec["host_ms_min_max"] = clocked(lambda: be.range_counts(W, thr, Xh), steps=2)
            rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del cc, counts
            torch.cuda.empty_cache()
        del Xt, Xh
        torch.cuda.empty_cache()
    be.release()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
