"""kneighbors (csrc/kneighbors.hip) against its two kernels and against what a user did before it, on the MI355X: one
JSON line per shape and k, also written to --out (default profiles/kneighbors_bench.json).

    python tools/bench_kneighbors.py [--steps 10] [--warmup 3] [--shapes 0,1,2] [--no-host]

Shapes (float32 rows generated in HBM, prototypes = rows plus noise): 1e6 x 784 with M = 1024 and M = 100, 1e5 x 64
with M = 25; k = 8 and k = 32 (M where M is smaller).  Each line, HIP events on one stream, median of --steps after
--warmup with [min, max], every figure of a line from the same process on the same GPU:
  T_d_ms        dbgsom_distances on the same buffers, writing the full N x M matrix (the parent's kernel)
  T_s_ms        dbgsom_topk_rows on one resident slab of slab_rows x M squared values
  T_k_ms        dbgsom_kneighbors, device time, at the default slab; slabs = ceil(N / slab_rows)
  bound_ms      1.1 * (T_d_ms + slabs * T_s_ms); within_bound = T_k_ms <= bound_ms
  slab_sweep    T_k_ms, T_s_ms and the bound with the slab at 16, 64 and 256 MiB (k of the line)
  call_ms       the whole HipBackend.kneighbors call on the device tensor (host clock), peak_bytes its torch peak plus
                the slab
  topk_ms       torch.topk(backend.distances(W, X), k, largest=False) on the same tensor (host clock) and its torch
                peak (topk_peak_bytes); same_as_topk: equal distances
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
SLABS_MIB = [16, 64, 256]


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def slab_rows_for(mib, N, M):
    ldr = M + M % 2
    return min(N, max(128, (mib << 20) // (ldr * 8) // 128 * 128))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kneighbors_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_kneighbors.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    be = HipBackend(0)
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
        out = torch.empty((N, M), dtype=torch.float64, device="cuda")
        td_ms, td_mm = timed(lambda: _native.call("dbgsom_distances", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(),
                                                  Wt.data_ptr(), M, ww.data_ptr(), out.data_ptr(), M, stream))
        ldr = M + M % 2
        rows_max = slab_rows_for(max(SLABS_MIB), N, M)
        R = torch.zeros((rows_max, ldr), dtype=torch.float64, device="cuda")
        R[:, :M] = out[:rows_max] ** 2
        del out
        torch.cuda.empty_cache()
        ws_bytes = lib.dbgsom_kneighbors_workspace_bytes(N, M, rows_max)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

        for k in sorted({min(8, M), min(32, M)}):
            idx = torch.empty((N, k), dtype=torch.int64, device="cuda")
            dist = torch.empty((N, k), dtype=torch.float64, device="cuda")

            def at_slab(rows):
                ts = timed(lambda: _native.call("dbgsom_topk_rows", R.data_ptr(), rows, M, ldr, k, idx.data_ptr(),
                                                dist.data_ptr(), stream))
                tk = timed(lambda: _native.call("dbgsom_kneighbors", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(),
                                                Wt.data_ptr(), M, ww.data_ptr(), k, rows, idx.data_ptr(), dist.data_ptr(),
                                                ws.data_ptr(), ws_bytes, stream))
                slabs = -(-N // rows)
                return ts, tk, slabs, round(1.1 * (td_ms + slabs * ts[0]), 4)

            sweep = {}
            for mib in SLABS_MIB:
                rows = slab_rows_for(mib, N, M)
                ts, tk, slabs, bound = at_slab(rows)
                sweep[str(mib)] = {"slab_rows": rows, "slabs": slabs, "T_s_ms": ts[0], "T_k_ms": tk[0],
                                   "T_k_ms_min_max": tk[1], "bound_ms": bound, "within_bound": bool(tk[0] <= bound)}
            default_rows = lib.dbgsom_kneighbors_workspace_bytes(N, M, 0) // ((M + M % 2) * 8)   # (a multiple of 128: exact)
            default_rows = min(N, default_rows)
            ts, tk, slabs, bound = at_slab(default_rows)
            del idx, dist
            torch.cuda.empty_cache()

            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            kd, ki = be.kneighbors(W, k, Xt)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base + lib.dbgsom_kneighbors_workspace_bytes(N, M, 0)
            call_ms, call_mm = clocked(lambda: be.kneighbors(W, k, Xt))
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tv, ti = torch.topk(be.distances(W, Xt), k, largest=False)
            torch.cuda.synchronize()
            topk_peak = torch.cuda.max_memory_allocated() - base
            same = bool(torch.equal(tv, kd))
            del tv, ti
            torch.cuda.empty_cache()
            topk_ms, topk_mm = clocked(lambda: torch.topk(be.distances(W, Xt), k, largest=False))
            torch.cuda.empty_cache()
            rec = {"N": N, "d": d, "M": M, "k": k, "dtype": "float32", "T_d_ms": td_ms, "T_d_ms_min_max": td_mm,
                   "slab_rows": default_rows, "slabs": slabs, "T_s_ms": ts[0], "T_s_ms_min_max": ts[1],
                   "T_k_ms": tk[0], "T_k_ms_min_max": tk[1], "bound_ms": bound, "within_bound": bool(tk[0] <= bound),
                   "slab_sweep": sweep, "call_ms": call_ms, "call_ms_min_max": call_mm, "peak_bytes": int(peak),
                   "topk_ms": topk_ms, "topk_ms_min_max": topk_mm, "topk_peak_bytes": int(topk_peak),
                   "same_as_topk": same, "matrix_bytes": N * M * 8}
            if not a.no_host:
                Xh = Xt.cpu().numpy()
                before = be.sample_traffic()
                hd, hi = be.kneighbors(W, k, Xh)
                after = be.sample_traffic()
                rec.update({"x_upload_bytes": after["x_upload_bytes"] - before["x_upload_bytes"],
                            "x_download_bytes": after["x_download_bytes"] - before["x_download_bytes"],
                            "host_equals_device": bool(np.array_equal(hi, ki.cpu().numpy()))})
                rec["host_ms"], rec["host_ms_min_max"] = clocked(lambda: be.kneighbors(W, k, Xh), steps=2)
                del Xh
            rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del kd, ki
        del Xt, R, ws
        torch.cuda.empty_cache()
    be.release()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
