"""The combined error (csrc/geodesics.hip) against the k = 2 query search it follows and the geodesics it reads, on the
MI355X: one JSON line per shape, also written to --out (default profiles/combined_error_bench.json).

    python tools/bench_combined_error.py [--steps 10] [--warmup 3] [--shapes 0,1] [--maps 1024,4096,16000] [--no-host]
                                         [--no-scipy]

Query shapes of the sibling tools (float32 rows generated in HBM, prototypes = rows plus noise, a sheet of M units as
square as M allows): 1e6 x 784 with M = 1024, 1e5 x 64 with M = 25.  Median of --steps after --warmup with [min, max];
the two sides of a comparison alternate inside one loop, every figure of a line from the same process on the same GPU.
The context calls run on the context's stream and return when it is idle, so they are timed by the host clock around the
blocking call (the device was idle before it); the raw calls by HIP events on the stream they are given.
  T_ce_ms     dbgsom_ctx_combined_error_query_device on the device rows
  T_k2_ms     dbgsom_ctx_bmu_query_device at k = 2, round_f32 = 0, on the same rows (the yardstick: existing code)
  T_geo_ms    dbgsom_geodesics alone over all M sources (edge lengths formed before, not timed)
  T_rows_ms   dbgsom_combined_error_rows alone on the N pairs of the search (a gather per row)
  bound_ms    1.1 * (T_k2 + T_geo); within_bound = T_ce_ms <= bound_ms; over_by names the part that costs it
  host_ms     the whole HipBackend.combined_error call on the same rows as a host array, with its PCIe bytes
Geodesics alone (one line per M of --maps, a sheet of M units): T_geo_ms, rounds of the synchronous restatement's bound
(the sheet's diameter), peak_bytes of the device (G, edges, lengths, workspace), and scipy_ms of
scipy.sparse.csgraph.dijkstra on the same graph on the host with equal_bits of the two matrices."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 784, 1024), (100_000, 64, 25)]


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def sheet(M):
    """-> (rows, cols, edges): the sheet of M units that is as square as M allows"""
    rows = max(r for r in range(1, int(np.sqrt(M)) + 1) if M % r == 0)
    cols = M // rows
    n = np.arange(M).reshape(rows, cols)
    right = np.stack([n[:, :-1].ravel(), n[:, 1:].ravel()], axis=1)
    down = np.stack([n[:-1].ravel(), n[1:].ravel()], axis=1)
    return rows, cols, np.ascontiguousarray(np.concatenate([right, down]), dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--maps", default="1024,4096,16000")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combined_error_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_combined_error.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    be = HipBackend(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def emit(rec):
        rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def clocked_pair(fa, fb, steps=None, warmup=None):
        """blocking calls, the two sides alternating, host clock"""
        steps, warmup = steps or a.steps, a.warmup if warmup is None else warmup
        ta, tb = [], []
        for _ in range(warmup + steps):
            for fn, t in ((fa, ta), (fb, tb)):
                if fn is None:
                    t.append(0.0)
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
        return med(ta[warmup:]), med(tb[warmup:])

    def timed(fn):
        """a raw call on torch's stream, HIP events"""
        t = []
        for _ in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return med(t[a.warmup:])

    def device_graph(W, edges):
        """-> (edges, lengths, workspace, its size) on the device; the lengths are the kernel's"""
        M, d = W.shape
        E = len(edges)
        Wt, et = torch.from_numpy(W).cuda(), torch.from_numpy(edges).cuda()
        lt = torch.empty(E, dtype=torch.float64, device="cuda")
        _native.call("dbgsom_edge_lengths", Wt.data_ptr(), M, d, d, et.data_ptr(), E, lt.data_ptr(), stream)
        nbytes = lib.dbgsom_geodesics_workspace_bytes(M, E)
        return et, lt, torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes

    for si in (int(s) for s in a.shapes.split(",") if s != ""):
        N, d, M = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        Xt = torch.randn(N, d, generator=g, device="cuda") + 3.0 * torch.randint(0, 8, (N, 1), generator=g, device="cuda")
        rng = np.random.default_rng(si)
        W = Xt[torch.from_numpy(rng.choice(N, M, replace=False)).cuda()].double().cpu().numpy()
        W += 0.05 * rng.standard_normal((M, d))
        rows, cols, edges = sheet(M)
        E = len(edges)
        idx2 = torch.empty((N, 2), dtype=torch.int64, device="cuda")
        dist2 = torch.empty((N, 2), dtype=torch.float64, device="cuda")
        units = torch.empty((N, 2), dtype=torch.int64, device="cuda")
        e = torch.empty(N, dtype=torch.float64, device="cuda")
        ctx = be._ctx

        def k2():
            _native.call("dbgsom_ctx_bmu_query_device", ctx, ctypes.c_void_p(Xt.data_ptr()), _native.F32, N, d, d,
                         W.ctypes.data, M, 2, 0, ctypes.c_void_p(idx2.data_ptr()), ctypes.c_void_p(dist2.data_ptr()))

        def combined():
            _native.call("dbgsom_ctx_combined_error_query_device", ctx, ctypes.c_void_p(Xt.data_ptr()), _native.F32, N, d,
                         d, W.ctypes.data, M, edges.ctypes.data, E, ctypes.c_void_p(units.data_ptr()),
                         ctypes.c_void_p(e.data_ptr()))

        (tk, tk_mm), (tc, tc_mm) = clocked_pair(k2, combined)
        same_units = bool(torch.equal(idx2, units))
        et, lt, ws, nbytes = device_graph(W, edges)
        G = torch.empty((M, M), dtype=torch.float64, device="cuda")

        def geo():
            _native.call("dbgsom_geodesics", et.data_ptr(), lt.data_ptr(), E, M, None, M, G.data_ptr(), M, ws.data_ptr(),
                         nbytes, stream)

        def rows_alone():
            _native.call("dbgsom_combined_error_rows", idx2.data_ptr(), dist2.data_ptr(), 2, N, G.data_ptr(), M, M,
                         e.data_ptr(), stream)

        e_ctx = e.clone()
        tg, tg_mm = timed(geo)
        tr, tr_mm = timed(rows_alone)
        torch.cuda.synchronize()
        same_e = bool(torch.equal(e.view(torch.int64), e_ctx.view(torch.int64)))
        bound = round(1.1 * (tk + tg), 4)
        rec = {"N": N, "d": d, "M": M, "sheet": [rows, cols], "E": E, "dtype": "float32",
               "T_ce_ms": tc, "T_ce_ms_min_max": tc_mm, "T_k2_ms": tk, "T_k2_ms_min_max": tk_mm,
               "T_geo_ms": tg, "T_geo_ms_min_max": tg_mm, "T_rows_ms": tr, "T_rows_ms_min_max": tr_mm,
               "bound_ms": bound, "within_bound": bool(tc <= bound), "same_units_as_k2": same_units,
               "raw_calls_give_the_same_e": same_e}
        if tc > bound:
            rec["over_by"] = {"ms": round(tc - bound, 4),
                              "costliest_part": max((("geodesic_kernel", tg), ("combined_error_rows_kernel", tr),
                                                     ("k = 2 search", tk)), key=lambda p: p[1])[0]}
        if not a.no_host:
            Xh = Xt.cpu().numpy()
            before = be.sample_traffic()
            he, hu = be.combined_error(W, edges, Xh)
            after = be.sample_traffic()
            rec.update({"x_upload_bytes": after["x_upload_bytes"] - before["x_upload_bytes"],
                        "x_download_bytes": after["x_download_bytes"] - before["x_download_bytes"],
                        "host_equals_device": bool(np.array_equal(hu, units.cpu().numpy())
                                                   and np.array_equal(he.view(np.int64), e_ctx.cpu().numpy().view(np.int64)))})
            (th, th_mm), _ = clocked_pair(lambda: be.combined_error(W, edges, Xh), None, steps=2, warmup=0)
            rec["host_ms"], rec["host_ms_min_max"] = th, th_mm
            del Xh
        emit(rec)
        del Xt, idx2, dist2, units, e, e_ctx, G, et, lt, ws
        torch.cuda.empty_cache()

    for M in (int(m) for m in a.maps.split(",") if m != ""):
        rows, cols, edges = sheet(M)
        E = len(edges)
        W = np.random.default_rng(M).normal(size=(M, 16))
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        et, lt, ws, nbytes = device_graph(W, edges)
        G = torch.empty((M, M), dtype=torch.float64, device="cuda")

        def geo():
            _native.call("dbgsom_geodesics", et.data_ptr(), lt.data_ptr(), E, M, None, M, G.data_ptr(), M, ws.data_ptr(),
                         nbytes, stream)

        tg, tg_mm = timed(geo)
        torch.cuda.synchronize()
        rec = {"geodesics_alone": True, "M": M, "sheet": [rows, cols], "E": E, "T_geo_ms": tg, "T_geo_ms_min_max": tg_mm,
               "rounds_bound": rows + cols - 2, "lds_bytes": M * 8, "lanes": 1024 if M * 8 > 65536 else 256,
               "peak_bytes": int(torch.cuda.max_memory_allocated() - base)}
        if not a.no_scipy:
            from scipy.sparse import csr_matrix
            from scipy.sparse.csgraph import dijkstra

            lens = lt.cpu().numpy()
            u, v = np.concatenate([edges[:, 0], edges[:, 1]]), np.concatenate([edges[:, 1], edges[:, 0]])
            A = csr_matrix((np.concatenate([lens, lens]), (u, v)), shape=(M, M))
            t0 = time.perf_counter()
            ref = dijkstra(A, directed=True)
            rec["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["equal_bits"] = bool(np.array_equal(G.cpu().numpy().view(np.int64), ref.view(np.int64)))
            rec["speedup"] = round(rec["scipy_ms"] / tg, 1)
            del ref
        emit(rec)
        del G, et, lt, ws
        torch.cuda.empty_cache()
    be.release()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
