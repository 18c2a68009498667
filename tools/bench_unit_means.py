"""Per-unit sums of a per-row quantity (csrc/unit_sums.hip) on the MI355X: the fold alone, ``unit_means`` from a tensor
against the k = 1 neighbour search it runs behind, ``torch.bincount`` for scale, the early-epoch case, and what
``target_statistics`` adds to a frozen-map epoch.  One JSON line per shape and V, also written to --out (default
profiles/unit_means_bench.json).

    python tools/bench_unit_means.py [--steps 10] [--warmup 3] [--shapes 0,1,2]

Shapes of the sibling tools (float32 rows generated in HBM, prototypes = rows plus noise): 1e6 x 784 with M = 1024 and
M = 100, 1e5 x 64 with M = 25; V = 1 and 16 float64 values per row, the units those of the k = 1 search.  The calls wait
for the context's stream themselves, so every figure is the host's clock around a call that returns after the device is
done (torch synchronised in front), median of --steps after --warmup with [min, max]; the two sides of a comparison
alternate inside one loop, every figure of a line from the same process on the same GPU:
  T_fold_ms       dbgsom_ctx_unit_sums_device on the tensors (sort, block sums, fold), no weights; T_fold_w_ms with weights
  T_k1_ms         est.kneighbors(X, 1) on the tensor (the yardstick: existing code on the same rows), alternating with
  T_means_ms      est.unit_means(X, Z) on the same tensor (the search, then the fold)
  ratio           T_means / T_k1; within_1p1 = ratio <= 1.1, the verdict; where it is missed `missed_by` names the part
                  that costs it: the fold's share (T_fold) or what lies around it
  T_bincount_ms   torch.bincount(units, weights=Z[:, 0], minlength=M): float atomics, no defined order, one column
  T_fold_m4_ms    the fold at M = 4 on the same N rows, random units (the early epochs: 2 x 2 map)
  T_epoch_ms      a frozen-map epoch on the resident rows, alternating with
  T_epoch_ts_ms   the same epoch followed by target_statistics(None, M, want_err=True) on the winners it left in HBM"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_means_bench.json"))
    a = ap.parse_args()
    import torch

    from dbgsom_amd import SomVQ, _native
    from dbgsom_amd.backend import RESIDENT, HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_unit_means.py measures on the MI355X: no GPU visible")
    _native.load()
    be = HipBackend(0)
    lines = []

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def timed(*fns):
        """the sides alternating: -> [(median, [min, max]) of each]"""
        ts = [[] for _ in fns]
        for _ in range(a.warmup + a.steps):
            for fn, t in zip(fns, ts):
                t.append(clock(fn))
        return [med(t[a.warmup:]) for t in ts]

    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for si in (int(s) for s in a.shapes.split(",")):
        N, d, M = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(si)
        Xt = torch.randn(N, d, generator=g, device="cuda") + 3.0 * torch.randint(0, 8, (N, 1), generator=g, device="cuda")
        rng = np.random.default_rng(si)
        W = Xt[torch.from_numpy(rng.choice(N, M, replace=False)).cuda()].double().cpu().numpy()
        W += 0.05 * rng.standard_normal((M, d))
        est = SomVQ(backend=be)
        est.weights_, est.n_features_in_, est.neurons_ = W, d, [(j, 0) for j in range(M)]
        units = est.kneighbors(Xt, 1, return_distance=False)[:, 0].contiguous()
        units4 = torch.randint(0, 4, (N,), generator=g, device="cuda")
        wt = torch.rand(N, generator=g, device="cuda", dtype=torch.float64)
        cols = max(1, int(np.sqrt(M)))
        xy = np.stack(np.divmod(np.arange(M), cols), axis=1)
        hop = np.abs(xy[:, None, :] - xy[None, :, :]).max(axis=2).astype(np.float64)
        gamma = 1.0 / float(Xt[:4096].double().var(dim=0).sum())
        for V in (1, 16):
            Zt = torch.randn(N, V, generator=g, device="cuda", dtype=torch.float64)
            mass = torch.empty(M, dtype=torch.float64, device="cuda")
            sums = torch.empty((M, V), dtype=torch.float64, device="cuda")

            def fold(u=units, w=None, m=M):
                _native.call("dbgsom_ctx_unit_sums_device", be._ctx, p(u), p(Zt), V, None if w is None else p(w), N, m, V,
                             p(mass), p(sums), V)

            (tf, tf_mm), (tfw, tfw_mm), (tf4, tf4_mm) = timed(fold, lambda: fold(w=wt), lambda: fold(u=units4, m=4))
            (tk, tk_mm), (tm, tm_mm) = timed(lambda: est.kneighbors(Xt, 1), lambda: est.unit_means(Xt, Zt))
            (tb, tb_mm), = timed(lambda: torch.bincount(units, weights=Zt[:, 0], minlength=M))
            fold()
            same = bool(torch.equal(est.unit_means(Xt, Zt).reshape(M, V), sums / mass[:, None]))
            be.load_device(Xt)
            be.set_targets(Zt)
            be.epoch(W, hop, 1.0, gamma, keep_on_device=True, frozen=True)

            def epoch():
                be.epoch(RESIDENT, hop, 1.0, gamma, keep_on_device=True, frozen=True)

            def epoch_ts():
                epoch()
                be.target_statistics(None, M, want_err=True)

            (te, te_mm), (tes, tes_mm) = timed(epoch, epoch_ts)
            be.release()
            within = bool(tm <= 1.1 * tk)
            rec = {"N": N, "d": d, "M": M, "V": V, "dtype": "float32",
                   "T_fold_ms": tf, "T_fold_ms_min_max": tf_mm, "T_fold_w_ms": tfw, "T_fold_w_ms_min_max": tfw_mm,
                   "T_k1_ms": tk, "T_k1_ms_min_max": tk_mm, "T_means_ms": tm, "T_means_ms_min_max": tm_mm,
                   "ratio": round(tm / tk, 4), "within_1p1": within,
                   "T_bincount_ms": tb, "T_bincount_ms_min_max": tb_mm, "T_fold_m4_ms": tf4, "T_fold_m4_ms_min_max": tf4_mm,
                   "fold_bytes_per_s": round(N * (8 + 4 + 8 * V) / (tf * 1e-3), 1),
                   "T_epoch_ms": te, "T_epoch_ms_min_max": te_mm, "T_epoch_ts_ms": tes, "T_epoch_ts_ms_min_max": tes_mm,
                   "target_statistics_ms": round(tes - te, 4), "raw_equals_call": same}
            if not within:
                rec["missed_by"] = ("unit_block_kernel and the sort in front of it (the fold)" if tf >= 0.5 * (tm - tk)
                                    else "the calls around the fold (validation, allocation, the division)")
            rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del Zt, mass, sums
        del Xt, units, units4, wt
        torch.cuda.empty_cache()
    be.release()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
