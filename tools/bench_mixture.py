"""The mixture view (csrc/mixture.hip) against the k = 1 neighbour search it is built beside, and against what a user
did before it, on the MI355X: one JSON line per shape, also written to --out (default profiles/mixture_bench.json).

    python tools/bench_mixture.py [--steps 10] [--warmup 3] [--shapes 0,1,2] [--no-host] [--no-torch]

Shapes of tools/bench_distortion.py (float32 rows generated in HBM, prototypes = rows plus noise): 1e6 x 784 with
M = 1024 and M = 100, 1e5 x 64 with M = 25; random priors, h^2 the mean squared quantization error per feature of the
first 4096 rows, Y the lattice coordinates of a square sheet.  HIP events on one stream, median of --steps after --warmup
with [min, max]; the two sides of a comparison alternate inside one loop, every figure of a line from the same process
on the same GPU:
  T_k1_ms        dbgsom_kneighbors at k = 1 on the same buffers, default slab (the yardstick: existing code, same slabs)
  T_mix0_ms      dbgsom_mixture with n_values = 0 on the same buffers (alternating with the yardstick)
  T_k1b_ms       the yardstick again, alternating with
  T_mix2_ms      dbgsom_mixture with n_values = 2
  ratio_V0       T_mix0 / T_k1; within_1p1 = ratio_V0 <= 1.1, the verdict; ratio_V2 = T_mix2 / T_k1b (recorded)
  T_s_ms         dbgsom_topk_rows (k = 1) on one resident slab of slab_rows x M squared values
  T_m0_ms        dbgsom_mixture_rows with n_values = 0 on the same slab; T_m2_ms with n_values = 2 (against T_sb_ms)
  rows_extra_ms  slabs * (T_m0 - T_s): what the rows kernel costs a call beyond the selection it replaces; where the
                 verdict is missed, `missed_by` names the kernel that share belongs to
  call_ms        the whole HipBackend.mixture call (n_values = 2) on the device tensor (host clock), peak_bytes its torch
                 peak plus the slab
  torch_ms       torch.logsumexp(a - c * D ** 2, 1) on D = backend.distances(W, X) (host clock), torch_peak_bytes its
                 torch peak; max_abs_diff of the two log-sums
  host_ms        the call on the same rows as a host array, with its PCIe bytes (x_upload_bytes, x_download_bytes)"""
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
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_mixture.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    be = HipBackend(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def timed_pair(fa, fb):
        """the two sides alternating: -> (median, [min, max]) of each"""
        ta, tb = [], []
        for _ in range(a.warmup + a.steps):
            for fn, t in ((fa, ta), (fb, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
        return med(ta[a.warmup:]), med(tb[a.warmup:])

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
        w = rng.random(M) + 0.05
        prior = np.log(w / w.sum())
        cols = max(1, int(np.sqrt(M)))
        Y = np.stack(np.divmod(np.arange(M), cols), axis=1).astype(np.float64)
        Wt, At, Yt = torch.from_numpy(W).cuda(), torch.from_numpy(prior).cuda(), torch.from_numpy(Y).cuda()
        head = be.kneighbors(W, 1, Xt[:4096])[0]
        c = 1.0 / (2.0 * float((head ** 2).mean()) / d)
        xx = torch.empty(N, dtype=torch.float64, device="cuda")
        ww = torch.empty(M, dtype=torch.float64, device="cuda")
        _native.call("dbgsom_row_sqnorms", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), stream)
        _native.call("dbgsom_row_sqnorms", Wt.data_ptr(), _native.F64, M, d, d, ww.data_ptr(), stream)
        ldr = M + M % 2
        ws_bytes = lib.dbgsom_kneighbors_workspace_bytes(N, M, 0)
        rows = min(N, ws_bytes // (ldr * 8))
        slabs = -(-N // rows)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        idx = torch.empty(N, dtype=torch.int64, device="cuda")
        dist = torch.empty(N, dtype=torch.float64, device="cuda")
        unit = torch.empty(N, dtype=torch.int64, device="cuda")
        lse = torch.empty(N, dtype=torch.float64, device="cuda")
        q = torch.empty((N, 2), dtype=torch.float64, device="cuda")

        def k1():
            _native.call("dbgsom_kneighbors", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                         ww.data_ptr(), 1, 0, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, stream)

        def mix(nv):
            _native.call("dbgsom_mixture", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                         ww.data_ptr(), At.data_ptr(), c, Yt.data_ptr() if nv else None, nv, 2 if nv else 0, 0,
                         unit.data_ptr(), lse.data_ptr(), q.data_ptr() if nv else None, 2 if nv else 0, ws.data_ptr(),
                         ws_bytes, stream)

        (tk, tk_mm), (t0, t0_mm) = timed_pair(k1, lambda: mix(0))
        (tkb, tkb_mm), (t2, t2_mm) = timed_pair(k1, lambda: mix(2))
        unit_raw, lse_raw, q_raw = unit.clone(), lse.clone(), q.clone()     # (the slab runs below write the heads again)
        # one resident slab: what the product kernel left in the workspace for the last slab's rows
        n_last = N - (slabs - 1) * rows
        R = ws.view(torch.float64)[: rows * ldr].view(rows, ldr)
        if n_last < rows:     # fill the slab with whole rows of squared values
            R[n_last:] = R[:n_last].repeat(-(-rows // n_last), 1)[: rows - n_last]

        def sel():
            _native.call("dbgsom_topk_rows", R.data_ptr(), rows, M, ldr, 1, idx.data_ptr(), dist.data_ptr(), stream)

        def ker(nv):
            _native.call("dbgsom_mixture_rows", R.data_ptr(), rows, M, ldr, At.data_ptr(), c, Yt.data_ptr() if nv else None,
                         nv, 2 if nv else 0, unit.data_ptr(), lse.data_ptr(), q.data_ptr() if nv else None, 2 if nv else 0,
                         stream)

        (ts, ts_mm), (tm0, tm0_mm) = timed_pair(sel, lambda: ker(0))
        (tsb, tsb_mm), (tm2, tm2_mm) = timed_pair(sel, lambda: ker(2))
        within = bool(t0 <= 1.1 * tk)
        rec = {"N": N, "d": d, "M": M, "dtype": "float32", "slab_rows": rows, "slabs": slabs, "c": c,
               "T_k1_ms": tk, "T_k1_ms_min_max": tk_mm, "T_mix0_ms": t0, "T_mix0_ms_min_max": t0_mm,
               "T_k1b_ms": tkb, "T_k1b_ms_min_max": tkb_mm, "T_mix2_ms": t2, "T_mix2_ms_min_max": t2_mm,
               "ratio_V0": round(t0 / tk, 4), "ratio_V2": round(t2 / tkb, 4), "within_1p1": within,
               "T_s_ms": ts, "T_s_ms_min_max": ts_mm, "T_m0_ms": tm0, "T_m0_ms_min_max": tm0_mm,
               "T_sb_ms": tsb, "T_sb_ms_min_max": tsb_mm, "T_m2_ms": tm2, "T_m2_ms_min_max": tm2_mm,
               "m0_over_s": round(tm0 / ts, 3), "m2_over_s": round(tm2 / tsb, 3),
               "m0_bytes_per_s": round(rows * 8 * M / (tm0 * 1e-3), 1),
               "rows_extra_ms": round(slabs * (tm0 - ts), 4)}
        if not within:
            rec["missed_by"] = "mixture_rows_kernel<0>" if slabs * (tm0 - ts) >= 0.5 * (t0 - tk) else "launch_distances_squared"
        del ws, R, idx, dist
        torch.cuda.empty_cache()

        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        cu, cl, cq = be.mixture(W, prior, c, Y, Xt)
        torch.cuda.synchronize()
        rec["peak_bytes"] = int(torch.cuda.max_memory_allocated() - base + ws_bytes)
        rec["call_ms"], rec["call_ms_min_max"] = clocked(lambda: be.mixture(W, prior, c, Y, Xt))
        rec["raw_equals_call"] = bool(torch.equal(cu, unit_raw) and torch.equal(cl, lse_raw) and torch.equal(cq, q_raw))
        del unit_raw, lse_raw, q_raw
        if not a.no_torch:
            def torch_route():
                D = be.distances(W, Xt)
                return torch.logsumexp(At - c * D ** 2, 1)

            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tl = torch_route()
            torch.cuda.synchronize()
            rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            rec["max_abs_diff"] = float((tl - cl).abs().max())
            del tl
            torch.cuda.empty_cache()
            rec["torch_ms"], rec["torch_ms_min_max"] = clocked(torch_route)
            torch.cuda.empty_cache()
        rec["matrix_bytes"] = N * M * 8
        if not a.no_host:
            Xh = Xt.cpu().numpy()
            before = be.sample_traffic()
            hu, hl, hq = be.mixture(W, prior, c, Y, Xh)
            after = be.sample_traffic()
            rec.update({"x_upload_bytes": after["x_upload_bytes"] - before["x_upload_bytes"],
                        "x_download_bytes": after["x_download_bytes"] - before["x_download_bytes"],
                        "host_equals_device": bool(np.array_equal(hu, cu.cpu().numpy()) and np.array_equal(hl, cl.cpu().numpy())
                                                   and np.array_equal(hq, cq.cpu().numpy()))})
            rec["host_ms"], rec["host_ms_min_max"] = clocked(lambda: be.mixture(W, prior, c, Y, Xh), steps=2)
            del Xh
        rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del Xt, cu, cl, cq, unit, lse, q
        torch.cuda.empty_cache()
    be.release()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
