"""Fit on rows with missing entries on the MI355X (csrc/masked.hip, csrc/masked_fit.hip, csrc/smooth.hip): one JSON
line per share of missing cells, also written to --out (default profiles/masked_fit_bench.json).

    python tools/bench_masked_fit.py [--fracs 0.01,0.1,0.5] [--steps 10] [--warmup 2] [--rows N] [--protos M]

The map is frozen: the same prototypes go into every step (a masked epoch takes them from the host each call anyway).
Each line:
  epoch_ms          HipBackend.epoch_masked on the resident rows, host clock around the blocking call (prototypes up,
                    search, sample kernel, sums, smoothing, new prototypes and the O(M) statistics down); median of --steps
  search_ms         HipBackend.bmu(W, 1) on the same residents (dbgsom_ctx_bmu_masked: n_obs and the float64 copy
                    were made at load), host clock; includes the download of N winners and distances
  sums_ms           dbgsom_accumulate_masked on the rows in HBM with the search's winners, HIP events on its stream
  smooth_ms         dbgsom_smooth_masked on those sums, HIP events
  plain_epoch_ms    for scale: the ordinary frozen epoch (HipBackend.epoch, aligned layout) on the rows with NaN set to 0
  segsum_ms         for scale: dbgsom_accumulate (segsum_kernel) on the zero-filled rows with the same winners, HIP events
  sums_over_segsum  sums_ms / segsum_ms on the same box and run: the masked kernel streams the same rows and writes a
                    slab three times as wide
  oracle_*          tests/masked_fit.py on the first --oracle-rows rows: differing winners, largest relative distance
                    difference
Data: tools/bench_missing.py's (seeded; 8 centres, rows and prototypes = a centre + N(0, 1), float32 rows, cells punched
out with probability frac, one random cell per row kept)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median_ms(fn, steps, warmup):
    t = [fn() for _ in range(warmup + steps)][warmup:]
    return round(float(np.median(t)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fracs", default="0.01,0.1,0.5")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--features", type=int, default=784)
    ap.add_argument("--protos", type=int, default=1024)
    ap.add_argument("--oracle-rows", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_fit_bench.json"))
    a = ap.parse_args()
    import torch

    from bench_missing import make
    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend
    from tests.test_missing_cpu import masked_bmu

    if not torch.cuda.is_available():
        raise SystemExit("bench_masked_fit.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, d, M = a.rows, a.features, a.protos
    side = int(np.sqrt(M))
    while M % side:
        side -= 1
    ii, jj = np.divmod(np.arange(M), M // side)
    hop = (np.abs(ii[:, None] - ii[None]) + np.abs(jj[:, None] - jj[None])).astype(np.float64)
    sigma = 2.0

    def timed(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    def walled(fn):
        def run():
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        return run

    lines = []
    for frac in (float(f) for f in a.fracs.split(",")):
        X, W = make(N, d, M, frac)
        gamma = float(np.nanvar(X, axis=0).sum() ** -1)
        hip = HipBackend(0).load(X, incomplete=True)
        epoch = median_ms(walled(lambda: hip.epoch_masked(W, hop, sigma, gamma)), a.steps, a.warmup)
        search = median_ms(walled(lambda: hip.bmu(W, 1)), a.steps, a.warmup)
        dist, win = hip.bmu(W, 1)
        hip.release()
        n_or = min(N, a.oracle_rows)
        want_dist, want_idx = masked_bmu(X[:n_or], W, 1)
        rel = float(np.max(np.abs(dist[:n_or] - want_dist) / np.where(want_dist > 0, want_dist, 1.0)))
        # the sums and the smoothing on their own, on device tensors
        kw = 1 - np.sqrt(1 - np.exp(-gamma * dist ** 2))
        Xt = torch.from_numpy(X).cuda()
        win_t, kw_t, dist_t = (torch.from_numpy(v).cuda() for v in (win, kw, dist))
        sums = torch.empty(M * (3 * d + 2), dtype=torch.float64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        nb = lib.dbgsom_accumulate_masked_workspace_bytes(N, d, M)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
        wsp = (ws.data_ptr() + 255) // 256 * 256
        sums_ms = median_ms(timed(lambda: _native.call(
            "dbgsom_accumulate_masked", Xt.data_ptr(), _native.F32, N, d, d, win_t.data_ptr(), kw_t.data_ptr(),
            dist_t.data_ptr(), M, sums.data_ptr(), status.data_ptr(), wsp, nb, stream)), a.steps, a.warmup)
        hop_t = torch.from_numpy(hop.astype(np.float32)).cuda()
        wo, wn = torch.from_numpy(W).cuda(), torch.empty((M, d), dtype=torch.float64, device="cuda")
        chg = torch.empty(1, dtype=torch.float64, device="cuda")
        nbs = lib.dbgsom_smooth_masked_workspace_bytes(M, d)
        wss = torch.empty(nbs + 256, dtype=torch.uint8, device="cuda")
        wssp = (wss.data_ptr() + 255) // 256 * 256
        smooth_ms = median_ms(timed(lambda: _native.call(
            "dbgsom_smooth_masked", sums.data_ptr(), M, d, hop_t.data_ptr(), sigma, wo.data_ptr(), wn.data_ptr(),
            chg.data_ptr(), wssp, nbs, stream)), a.steps, a.warmup)
        # for scale: segsum_kernel and the ordinary epoch on the zero-filled rows
        X0 = np.nan_to_num(X, nan=0.0)
        Xt.copy_(torch.from_numpy(X0))
        sums0 = torch.empty(M * (d + 3), dtype=torch.float64, device="cuda")
        nb0 = lib.dbgsom_accumulate_workspace_bytes(N, d, M)
        ws0 = torch.empty(nb0 + 256, dtype=torch.uint8, device="cuda")
        ws0p = (ws0.data_ptr() + 255) // 256 * 256
        segsum_ms = median_ms(timed(lambda: _native.call(
            "dbgsom_accumulate", Xt.data_ptr(), _native.F32, N, d, d, win_t.data_ptr(), kw_t.data_ptr(),
            dist_t.data_ptr(), M, sums0.data_ptr(), status.data_ptr(), ws0p, nb0, stream)), a.steps, a.warmup)
        del Xt, ws, ws0, wss
        plain = HipBackend(0).load(X0)
        plain_ms = median_ms(walled(lambda: plain.epoch(W, hop, sigma, gamma, "aligned", frozen=True)), a.steps, a.warmup)
        plain.release()
        line = {"N": N, "d": d, "M": M, "dtype": "float32", "missing": frac, "epoch_ms": epoch, "search_ms": search,
                "sums_ms": sums_ms, "smooth_ms": smooth_ms, "plain_epoch_ms": plain_ms, "segsum_ms": segsum_ms,
                "sums_over_segsum": round(sums_ms / segsum_ms, 2), "epoch_over_plain": round(epoch / plain_ms, 2),
                "oracle_rows": n_or, "oracle_max_rel_dist_diff": rel,
                "oracle_winners_differing": int(np.count_nonzero(win[:n_or] != want_idx)),
                "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
