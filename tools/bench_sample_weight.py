"""Frozen-map epoch with sample weights on a bench workload, one JSON line per workload:
unweighted / weighted with all ones / weighted with integer weights 1 .. 3 against the same epoch on the
repeated rows (torch.repeat_interleave(X, w)) / weights 0 .. 2 (a third of the rows at 0), whole epoch and the
accumulate stage alone.
    python tools/bench_sample_weight.py c4 [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from dbgsom_amd.backend import RESIDENT, HipBackend  # noqa: E402


def run(hip, hop, sigma, gamma, steps, warmup):
    """-> (ms per epoch: median wall clock of the blocking call, median ms of the accumulate stage)"""
    hip._set("timing", 1)
    wall, acc = [], []
    for e in range(warmup + steps):
        hip.phase_log = []
        t0 = time.perf_counter()
        hip.epoch(RESIDENT, hop, sigma, gamma, "compact", False, keep_on_device=True, frozen=True)
        if e >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            acc.append(hip.phase_log[-1][1])
    return float(np.median(wall)), float(np.median(acc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["c4"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.workloads:
        n, d, rows, cols, seed, kind, _ = bench.WORKLOADS[name]
        M = rows * cols
        X = bench.make_shard(torch, n, d, seed, dev, 0, kind)
        g = torch.Generator(device=dev).manual_seed(seed + 7)
        W = X[torch.randperm(n, device=dev, generator=g)[:M]].double().cpu().numpy()
        gamma = float(1.0 / X.double().var(dim=0, unbiased=False).sum().item())
        hop, sigma = bench.lattice_hops(rows, cols), 0.2 * np.sqrt(M)
        w = np.random.default_rng(seed).integers(1, 4, n)
        out = {"workload": name, "N": n, "d": d, "M": M, "sum_w": int(w.sum()), "steps": args.steps}
        hip = HipBackend(0).load_device(X)
        hip.set_weights(W)
        out["unweighted_ms"], out["unweighted_accumulate_ms"] = run(hip, hop, sigma, gamma, args.steps, args.warmup)
        hip.set_sample_weight(np.ones(n))
        out["weighted_ones_ms"], out["weighted_ones_accumulate_ms"] = run(hip, hop, sigma, gamma, args.steps, args.warmup)
        hip.set_sample_weight(w)
        out["weighted_int_ms"], out["weighted_int_accumulate_ms"] = run(hip, hop, sigma, gamma, args.steps, args.warmup)
        # a third of the rows at weight 0: they leave the sums, and the next search visits them last, unsorted
        wz = np.random.default_rng(seed + 1).integers(0, 3, n)
        hip.set_sample_weight(wz)
        out["rows_of_weight_0"] = int((wz == 0).sum())
        out["weighted_zero_third_ms"], out["weighted_zero_third_accumulate_ms"] = run(hip, hop, sigma, gamma, args.steps, args.warmup)
        hip.release()
        Xr = torch.repeat_interleave(X, torch.from_numpy(w).to(dev), dim=0)
        del X
        hip = HipBackend(0).load_device(Xr)
        hip.set_weights(W)
        out["repeated_rows_ms"], out["repeated_rows_accumulate_ms"] = run(hip, hop, sigma, gamma, args.steps, args.warmup)
        hip.release()
        out["weighted_over_repeated"] = out["weighted_int_ms"] / out["repeated_rows_ms"]
        out["weighted_over_repeated_accumulate"] = out["weighted_int_accumulate_ms"] / out["repeated_rows_accumulate_ms"]
        out["N_over_sum_w"] = n / float(w.sum())
        print(json.dumps(out), flush=True)
        del Xr


if __name__ == "__main__":
    main()
