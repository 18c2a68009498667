"""The nearest stored rows through the map (csrc/row_neighbors.hip) on the MI355X: the unit search and the scan of the
probed cells, against a plain gather of the same candidate rows and against an exact search.  One JSON line per shape,
number of queries and n_probe, also written to --out (default profiles/row_neighbors_bench.json).

    python tools/bench_row_neighbors.py [--steps 5] [--warmup 1] [--shapes 0,1] [--queries 1,10000] [--probes 1,8,32]

Shapes: 1e6 x 784 float32 with M = 1024, and 1e5 x 64 with M = 25 (rows generated in HBM: unit normal noise around
eight offsets; the prototypes are rows plus noise, not a trained map; the queries are rows plus noise of the size of the
rows' own).  k = 10; n_probe is capped at M.  X is indexed once per shape (load_device + partition).

Clock: everything timed runs on the context's stream between two HIP events, the stream waited for before the second is
recorded -- the context calls wait for their kernels themselves, and the gather is held to the same protocol; the two
sides of the verdict alternate inside one loop; median of --steps after --warmup with [min, max].
  T_units_ms      dbgsom_ctx_kneighbors_query_device at k = n_probe on the queries (the prototypes go up per call)
  T_scan_ms       dbgsom_ctx_scan_cells_device on the resident rows, the partition and those probe lists
  candidates      candidate rows of all queries together; cand_rows_per_s and cand_bytes_per_s: of the scan
  T_gather_ms     torch.index_select of the same candidate rows, in the same order, into a scratch buffer of at most
                  --scratch-rows rows (in pieces where they are more); ratio = T_scan / T_gather; within_margin:
                  ratio <= 1.1.  The scan reads what the gather reads and writes nothing.
  missed_by       for a line outside the margin: what the figures of the line say costs it
  recall_at_10    on 256 queries of their own: the share of the exact 10 nearest rows (torch.cdist in float64 plus
                  topk, over chunks of rows of X) that row_neighbors lists; exact_ms and exact_peak_bytes: that exact
                  search for the 256 queries (host clock, torch's peak)
  call_ms         HipBackend.row_neighbors on the query tensor (host clock); host_ms the same on a host array, with its
                  PCIe bytes (x_upload_bytes, x_download_bytes)"""
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
MARGIN = 1.1
K = 10


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--queries", default="1,10000")
    ap.add_argument("--probes", default="1,8,32")
    ap.add_argument("--scratch-rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_neighbors_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_row_neighbors.py measures on the MI355X: no GPU visible")
    _native.load()
    be = HipBackend(0)
    lines = []
    ext = None   # the context's stream (a release makes a new context: looked up per shape)

    def timed(*fns):
        """the sides alternating on the context's stream: -> (median, [min, max]) of each"""
        ts = [[] for _ in fns]
        for _ in range(a.warmup + a.steps):
            for fn, t in zip(fns, ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ext)
                fn()
                ext.synchronize()
                e1.record(ext)
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
        torch.cuda.synchronize()
        be.load_device(Xt)
        raw = ctypes.c_void_p()
        _native.call("dbgsom_ctx_stream", be._ctx, ctypes.byref(raw))
        ext = torch.cuda.ExternalStream(raw.value, device=torch.device("cuda", 0))
        be.partition(W)
        order_h, seg_h = be.read_partition()
        order_t = torch.from_numpy(order_h.astype(np.int64)).cuda()
        order32, seg32 = torch.from_numpy(order_h).cuda(), torch.from_numpy(seg_h.view(np.int32)).cuda()
        seg_t = torch.from_numpy(seg_h.astype(np.int64)).cuda()

        def queries(n, seed):
            gq = torch.Generator(device="cuda").manual_seed(1000 * si + seed)
            rows = torch.randint(0, N, (n,), generator=gq, device="cuda")
            return (Xt[rows] + torch.randn(n, d, generator=gq, device="cuda")).contiguous()

        # the exact search of the recall queries, once per shape
        Qr = queries(256, 7)

        def exact():
            best_d, best_i = None, None
            Qd = Qr.double()
            for r0 in range(0, N, 100_000):
                D = torch.cdist(Qd, Xt[r0:r0 + 100_000].double())
                dd, ii = torch.topk(D, K, dim=1, largest=False)
                ii = ii + r0
                best_d = dd if best_d is None else torch.cat([best_d, dd], 1)
                best_i = ii if best_i is None else torch.cat([best_i, ii], 1)
            dd, pos = torch.topk(best_d, K, dim=1, largest=False)
            return torch.gather(best_i, 1, pos)

        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        truth = exact()
        torch.cuda.synchronize()
        exact_peak = int(torch.cuda.max_memory_allocated() - base)
        exact_ms, exact_mm = clocked(exact, steps=2)
        truth_h = truth.cpu().numpy()

        for n_probe in sorted({min(int(p), M) for p in a.probes.split(",")}):
            got = be.row_neighbors(W, K, n_probe, Qr)[1].cpu().numpy()
            recall = float(np.mean([len(set(got[q]) & set(truth_h[q])) / K for q in range(256)]))
            for Nq in (int(s) for s in a.queries.split(",")):
                Q = queries(Nq, Nq)
                units = torch.empty((Nq, n_probe), dtype=torch.int64, device="cuda")
                udist = torch.empty((Nq, n_probe), dtype=torch.float64, device="cuda")
                idx = torch.empty((Nq, K), dtype=torch.int64, device="cuda")
                dist = torch.empty((Nq, K), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()

                def unit_search():
                    _native.call("dbgsom_ctx_kneighbors_query_device", be._ctx, Q.data_ptr(), _native.F32, Nq, d, d,
                                 W.ctypes.data, M, n_probe, units.data_ptr(), udist.data_ptr())

                def scan():
                    _native.call("dbgsom_ctx_scan_cells_device", be._ctx, Xt.data_ptr(), _native.F32, N, d, d,
                                 order32.data_ptr(), seg32.data_ptr(), M, Q.data_ptr(), _native.F32, Nq, d, units.data_ptr(),
                                 n_probe, K, idx.data_ptr(), dist.data_ptr())

                unit_search()
                # the candidate rows of all queries in scan order, as one list of row numbers on the device
                starts, ends = seg_t[units], seg_t[units + 1]
                lens = (ends - starts).reshape(-1)
                total = int(lens.sum())
                first = torch.cumsum(lens, 0) - lens
                pos = torch.arange(total, device="cuda") - torch.repeat_interleave(first, lens) \
                    + torch.repeat_interleave(starts.reshape(-1), lens)
                ids = order_t[pos]
                del pos, first
                piece = min(max(total, 1), a.scratch_rows)
                scratch = torch.empty((piece, d), dtype=torch.float32, device="cuda")

                def gather():
                    with torch.cuda.stream(ext):
                        for r0 in range(0, total, piece):
                            n = min(piece, total - r0)
                            torch.index_select(Xt, 0, ids[r0:r0 + n], out=scratch[:n])

                (tu, tu_mm), = timed(unit_search)
                (ts, ts_mm), (tg, tg_mm) = timed(scan, gather)
                cand_bytes = total * d * 4
                rec = {"N": N, "d": d, "M": M, "Nq": Nq, "k": K, "n_probe": n_probe, "dtype": "float32",
                       "T_units_ms": tu, "T_units_ms_min_max": tu_mm, "T_scan_ms": ts, "T_scan_ms_min_max": ts_mm,
                       "candidates": total, "candidates_per_query": round(total / Nq, 1),
                       "cand_rows_per_s": round(total / (ts * 1e-3), 1), "cand_bytes_per_s": round(cand_bytes / (ts * 1e-3), 1),
                       "T_gather_ms": tg, "T_gather_ms_min_max": tg_mm, "gather_bytes_per_s": round(cand_bytes / (tg * 1e-3), 1),
                       "gather_pieces": -(-total // piece), "ratio": round(ts / tg, 3), "margin": MARGIN,
                       "within_margin": bool(ts <= MARGIN * tg)}
                if not rec["within_margin"]:
                    rec["missed_by"] = (
                        "scan_cells_kernel: %.1f GB/s of candidate rows against the gather's %.1f GB/s read; one workgroup "
                        "per query (%d workgroups, %.0f candidates each, on 256 CUs), and per candidate row %d dependent "
                        "float64 steps per lane and six shuffle rounds behind loads of 4 bytes per lane"
                        % (cand_bytes / ts / 1e6, cand_bytes / tg / 1e6, Nq, total / Nq, -(-d // 64)))
                rec.update({"recall_at_10": round(recall, 4), "recall_queries": 256, "exact_ms": exact_ms,
                            "exact_ms_min_max": exact_mm, "exact_peak_bytes": exact_peak})
                del scratch, ids
                torch.cuda.empty_cache()
                dd, ii = be.row_neighbors(W, K, n_probe, Q)
                rec["call_equals_raw"] = bool(torch.equal(ii, idx) and torch.equal(dd, dist))
                rec["call_ms"], rec["call_ms_min_max"] = clocked(lambda: be.row_neighbors(W, K, n_probe, Q))
                Qh = Q.cpu().numpy()
                before = be.sample_traffic()
                hd, hi = be.row_neighbors(W, K, n_probe, Qh)
                after = be.sample_traffic()
                rec.update({"x_upload_bytes": after["x_upload_bytes"] - before["x_upload_bytes"],
                            "x_download_bytes": after["x_download_bytes"] - before["x_download_bytes"],
                            "host_equals_device": bool(np.array_equal(hi, ii.cpu().numpy()))})
                rec["host_ms"], rec["host_ms_min_max"] = clocked(lambda: be.row_neighbors(W, K, n_probe, Qh), steps=2)
                rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
                print(json.dumps(rec), flush=True)
                lines.append(rec)
        be.release()
        del Xt, order_t, order32, seg32, seg_t
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
