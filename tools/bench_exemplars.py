"""The k nearest rows to every prototype (csrc/exemplars.hip) against the neighbour search at the same k that it is built
beside, and against what a user did before it, on the MI355X: one JSON line per shape and k, also written to --out
(default profiles/exemplars_bench.json).

    python tools/bench_exemplars.py [--steps 10] [--warmup 3] [--shapes 0,1,2] [--ks 1,8,32] [--no-host] [--no-torch]

Shapes of tools/bench_kneighbors.py (float32 rows generated in HBM, prototypes = rows plus noise): 1e6 x 784 with
M = 1024 and M = 100, 1e5 x 64 with M = 25.  HIP events on one stream, median of --steps after --warmup with [min, max];
the two sides of a comparison alternate inside one loop, every figure of a line from the same process on the same GPU.
Both selections read the slab once from cache behind the same product kernel, so the yardstick of the device time is
dbgsom_kneighbors at the same k, existing code; the margin is 10 %, and a line that misses it says so and names the kernels
that cost it:
  T_kn_ms       dbgsom_kneighbors at k on the same buffers, default slab (the yardstick)
  T_X_ms        dbgsom_exemplars at k, own_cell off; T_Xown_ms with own_cell on (one more selection at k = 1 per slab)
  ratio, ratio_own       T_X / T_kn, T_Xown / T_kn; within_margin, own_within_margin: ratio <= 1.1
  T_rows_ms     dbgsom_topk_rows at k on one resident slab of slab_rows x M squared values
  T_fold_ms     dbgsom_topk_cols on the same slab (both kernels of the fold); T_fold_own_ms with the owners of the slab's
                rows; fold_over_rows = T_fold / T_rows; scratch_bytes: what the fold writes and reads per slab
  missed_by     for a line outside the margin: the kernels whose time on a slab exceeds the row selection's
  call_ms       the whole HipBackend.exemplars call on the device tensor (host clock), peak_bytes its torch peak plus the
                workspace of dbgsom_exemplars
  torch_ms      torch.topk(backend.distances(W, X).T, k, largest=False) (host clock), torch_peak_bytes its torch peak;
                same_dist: equal distances (the indices differ where topk breaks ties as it pleases: idx_equal_fraction)
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
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exemplars_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_exemplars.py measures on the MI355X: no GPU visible")
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
        rows = min(N, lib.dbgsom_kneighbors_workspace_bytes(N, M, 0) // (ldr * 8))
        slabs = -(-N // rows)
        Xh = None if a.no_host else Xt.cpu().numpy()
        for k in (int(s) for s in a.ks.split(",")):
            ws_bytes = lib.dbgsom_exemplars_workspace_bytes(N, M, k, 0)   # (covers that of dbgsom_kneighbors)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            kk = min(k, M)
            idx = torch.empty(N * kk, dtype=torch.int64, device="cuda")
            dist = torch.empty(N * kk, dtype=torch.float64, device="cuda")
            xi = torch.empty((2, M * k), dtype=torch.int64, device="cuda")
            xd = torch.empty((2, M * k), dtype=torch.float64, device="cuda")

            def kn():
                _native.call("dbgsom_kneighbors", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                             ww.data_ptr(), kk, 0, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, stream)

            def exemplars(own):
                _native.call("dbgsom_exemplars", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                             ww.data_ptr(), k, own, 0, xi[own].data_ptr(), xd[own].data_ptr(), ws.data_ptr(), ws_bytes,
                             stream)

            (tk, tk_mm), (tx, tx_mm), (to, to_mm) = timed(kn, lambda: exemplars(0), lambda: exemplars(1))
            # one resident slab: what the product kernel left in the workspace for the last slab's rows
            n_last = N - (slabs - 1) * rows
            R = ws.view(torch.float64)[: rows * ldr].view(rows, ldr)
            if n_last < rows:     # fill the slab with whole rows of squared values
                R[n_last:] = R[:n_last].repeat(-(-rows // n_last), 1)[: rows - n_last]
            scratch_bytes = lib.dbgsom_topk_cols_workspace_bytes(rows, M, k)
            scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device="cuda")
            sr = torch.empty(M * k, dtype=torch.float64, device="cuda")
            st = torch.empty(M * k, dtype=torch.int64, device="cuda")
            own_rows = torch.empty(rows, dtype=torch.int64, device="cuda")
            own_dist = torch.empty(rows, dtype=torch.float64, device="cuda")
            _native.call("dbgsom_topk_rows", R.data_ptr(), rows, M, ldr, 1, own_rows.data_ptr(), own_dist.data_ptr(), stream)
            _native.call("dbgsom_topk_cols_init", sr.data_ptr(), st.data_ptr(), M, k, stream)

            def sel_rows():
                _native.call("dbgsom_topk_rows", R.data_ptr(), rows, M, ldr, kk, idx.data_ptr(), dist.data_ptr(), stream)

            def fold(owner):
                _native.call("dbgsom_topk_cols", R.data_ptr(), rows, M, ldr, owner, 0, k, sr.data_ptr(), st.data_ptr(),
                             scratch.data_ptr(), scratch_bytes, stream)

            (tr, tr_mm), (tf, tf_mm), (tfo, tfo_mm) = timed(sel_rows, lambda: fold(None), lambda: fold(own_rows.data_ptr()))
            rec = {"N": N, "d": d, "M": M, "k": k, "dtype": "float32", "slab_rows": rows, "slabs": slabs,
                   "T_kn_ms": tk, "T_kn_ms_min_max": tk_mm, "T_X_ms": tx, "T_X_ms_min_max": tx_mm,
                   "T_Xown_ms": to, "T_Xown_ms_min_max": to_mm,
                   "ratio": round(tx / tk, 3), "ratio_own": round(to / tk, 3), "margin": MARGIN,
                   "within_margin": bool(tx <= MARGIN * tk), "own_within_margin": bool(to <= MARGIN * tk),
                   "T_rows_ms": tr, "T_rows_ms_min_max": tr_mm, "T_fold_ms": tf, "T_fold_ms_min_max": tf_mm,
                   "T_fold_own_ms": tfo, "T_fold_own_ms_min_max": tfo_mm, "fold_over_rows": round(tf / tr, 3),
                   "scratch_bytes": int(scratch_bytes), "slab_bytes": int(rows * ldr * 8)}
            missed = []
            if not rec["within_margin"]:
                missed.append("topk_cols_partial_kernel + topk_cols_merge_kernel: %.4f ms per slab against %.4f ms of "
                              "topk_rows_kernel" % (tf, tr))
            if not rec["own_within_margin"]:
                missed.append("own_cell: topk_rows_kernel<1> + the fold with owners, %.4f ms per slab above the row "
                              "selection" % ((to - tk) / slabs))
            if missed:
                rec["missed_by"] = missed
            del ws, R, idx, dist, scratch
            torch.cuda.empty_cache()

            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            cd, ci = be.exemplars(W, k, Xt)
            torch.cuda.synchronize()
            rec["peak_bytes"] = int(torch.cuda.max_memory_allocated() - base + ws_bytes)
            rec["device_call_equals_raw"] = bool(torch.equal(ci.ravel(), xi[0]) and torch.equal(cd.ravel(), xd[0]))
            rec["call_ms"], rec["call_ms_min_max"] = clocked(lambda: be.exemplars(W, k, Xt))
            rec["call_own_ms"], rec["call_own_ms_min_max"] = clocked(lambda: be.exemplars(W, k, Xt, own_cell=True))
            if not a.no_torch:
                def torch_route():
                    return torch.topk(be.distances(W, Xt).T, k, largest=False)

                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                tv, ti = torch_route()
                torch.cuda.synchronize()
                rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
                rec["same_dist"] = bool(torch.equal(tv, cd))
                rec["idx_equal_fraction"] = float((ti == ci).double().mean())
                del tv, ti
                torch.cuda.empty_cache()
                rec["torch_ms"], rec["torch_ms_min_max"] = clocked(torch_route)
                torch.cuda.empty_cache()
            rec["matrix_bytes"] = N * M * 8
            if Xh is not None:
                before = be.sample_traffic()
                hd, hi = be.exemplars(W, k, Xh)
                after = be.sample_traffic()
                rec.update({"x_upload_bytes": after["x_upload_bytes"] - before["x_upload_bytes"],
                            "x_download_bytes": after["x_download_bytes"] - before["x_download_bytes"],
                            "host_equals_device": bool(np.array_equal(hi, ci.cpu().numpy())
                                                       and np.array_equal(hd, cd.cpu().numpy()))})
                rec["host_ms"], rec["host_ms_min_max"] = clocked(lambda: be.exemplars(W, k, Xh), steps=2)
            rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del cd, ci, xi, xd
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
