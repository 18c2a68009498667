"""The distortion measure (csrc/distortion.hip) against the k = 1 neighbour search it is built beside, and against what a
user did before it, on the MI355X: one JSON line per shape, also written to --out (default
profiles/distortion_bench.json).

    python tools/bench_distortion.py [--steps 10] [--warmup 3] [--shapes 0,1,2] [--no-host] [--no-torch]

Shapes of tools/bench_kneighbors.py (float32 rows generated in HBM, prototypes = rows plus noise): 1e6 x 784 with
M = 1024 and M = 100, 1e5 x 64 with M = 25; H the Gaussian factors of a square sheet of M units.  HIP events on one
stream, median of --steps after --warmup with [min, max]; the two sides of a comparison alternate inside one loop, every
figure of a line from the same process on the same GPU:
  T_k1_ms       dbgsom_kneighbors at k = 1 on the same buffers, default slab (the yardstick: existing code, same slabs)
  T_E_ms        dbgsom_neighborhood_energy on the same buffers
  T_s_ms        dbgsom_topk_rows (k = 1) on one resident slab of slab_rows x M squared values
  T_e_ms        dbgsom_energy_rows on the same slab; e_bytes_per_s: two rows of 8 M bytes per sample over T_e
  e_over_s      T_e / T_s (recorded, not gated)
  bound_ms      1.1 * (T_k1 + slabs * (T_e - T_s)); within_bound = T_E_ms <= bound_ms
  call_ms       the whole HipBackend.neighborhood_energy call on the device tensor (host clock), peak_bytes its torch peak
                plus the slab and H
  torch_ms      (H_dev[D.argmin(1)] * D ** 2).sum(1) on D = backend.distances(W, X) (host clock), torch_peak_bytes its
                torch peak; same_bmu: equal units; max_rel_diff of the two e
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


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def sheet_factors(M, sigma=1.5):
    cols = max(1, int(np.sqrt(M)))
    ii, jj = np.divmod(np.arange(M), cols)
    hop = (np.abs(ii[:, None] - ii[None]) + np.abs(jj[:, None] - jj[None])).astype(np.float64)
    return np.exp(-(hop ** 2 / (2 * sigma ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_distortion.py measures on the MI355X: no GPU visible")
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
        H = sheet_factors(M)
        Wt, Ht = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
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
        bmu = torch.empty(N, dtype=torch.int64, device="cuda")
        e = torch.empty(N, dtype=torch.float64, device="cuda")

        def k1():
            _native.call("dbgsom_kneighbors", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(), M,
                         ww.data_ptr(), 1, 0, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, stream)

        def energy():
            _native.call("dbgsom_neighborhood_energy", Xt.data_ptr(), _native.F32, N, d, d, xx.data_ptr(), Wt.data_ptr(),
                         M, ww.data_ptr(), Ht.data_ptr(), M, 0, bmu.data_ptr(), e.data_ptr(), ws.data_ptr(), ws_bytes,
                         stream)

        (tk, tk_mm), (tE, tE_mm) = timed_pair(k1, energy)
        same_units = bool(torch.equal(idx, bmu))
        # one resident slab: what the product kernel left in the workspace for the last slab's rows
        n_last = N - (slabs - 1) * rows
        R = ws.view(torch.float64)[: rows * ldr].view(rows, ldr)
        if n_last < rows:     # fill the slab with whole rows of squared values
            R[n_last:] = R[:n_last].repeat(-(-rows // n_last), 1)[: rows - n_last]

        def sel():
            _native.call("dbgsom_topk_rows", R.data_ptr(), rows, M, ldr, 1, idx.data_ptr(), dist.data_ptr(), stream)

        def ker():
            _native.call("dbgsom_energy_rows", R.data_ptr(), rows, M, ldr, Ht.data_ptr(), M, bmu.data_ptr(), e.data_ptr(),
                         stream)

        (ts, ts_mm), (te, te_mm) = timed_pair(sel, ker)
        bound = round(1.1 * (tk + slabs * (te - ts)), 4)
        rec = {"N": N, "d": d, "M": M, "dtype": "float32", "slab_rows": rows, "slabs": slabs,
               "T_k1_ms": tk, "T_k1_ms_min_max": tk_mm, "T_E_ms": tE, "T_E_ms_min_max": tE_mm,
               "T_s_ms": ts, "T_s_ms_min_max": ts_mm, "T_e_ms": te, "T_e_ms_min_max": te_mm,
               "e_over_s": round(te / ts, 3), "e_bytes_per_s": round(rows * 2 * 8 * M / (te * 1e-3), 1),
               "bound_ms": bound, "within_bound": bool(tE <= bound), "same_units_as_k1": same_units}
        del ws, R, idx, dist, bmu, e
        torch.cuda.empty_cache()

        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ce, cb = be.neighborhood_energy(W, H, Xt)
        torch.cuda.synchronize()
        rec["peak_bytes"] = int(torch.cuda.max_memory_allocated() - base + ws_bytes + H.nbytes)
        rec["call_ms"], rec["call_ms_min_max"] = clocked(lambda: be.neighborhood_energy(W, H, Xt))
        if not a.no_torch:
            def torch_route():
                D = be.distances(W, Xt)
                b = D.argmin(1)
                return (Ht[b] * D ** 2).sum(1), b

            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            te_, tb_ = torch_route()
            torch.cuda.synchronize()
            rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            rec["same_bmu"] = bool(torch.equal(tb_, cb))
            rec["max_rel_diff"] = float(((te_ - ce).abs() / ce.abs().clamp_min(1e-300)).max())
            del te_, tb_
            torch.cuda.empty_cache()
            rec["torch_ms"], rec["torch_ms_min_max"] = clocked(torch_route)
            torch.cuda.empty_cache()
        rec["matrix_bytes"] = N * M * 8
        if not a.no_host:
            Xh = Xt.cpu().numpy()
            before = be.sample_traffic()
            he, hb = be.neighborhood_energy(W, H, Xh)
            after = be.sample_traffic()
            rec.update({"x_upload_bytes": after["x_upload_bytes"] - before["x_upload_bytes"],
                        "x_download_bytes": after["x_download_bytes"] - before["x_download_bytes"],
                        "host_equals_device": bool(np.array_equal(hb, cb.cpu().numpy())
                                                   and np.array_equal(he, ce.cpu().numpy()))})
            rec["host_ms"], rec["host_ms_min_max"] = clocked(lambda: be.neighborhood_energy(W, H, Xh), steps=2)
            del Xh
        rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del Xt, ce, cb
        torch.cuda.empty_cache()
    be.release()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
