"""The covariance pass of init="pca" (csrc/covariance.hip) on the MI355X against two yardsticks the library had before
it, and the whole start against a whole fit: one JSON line per shape, also written to --out (default
profiles/linear_init_bench.json).

    python tools/bench_linear_init.py [--steps 10] [--warmup 3] [--shapes 0,1] [--no-fit] [--no-eigh]

Shapes: 1e6 x 784 and 1e5 x 64, float32 rows generated in HBM as bench.py generates its clustered workloads (32 centres
~ N(0, 16 I), unit noise).  Each line, HIP events on one stream, median of --steps after --warmup with [min, max], every
figure of a line from the same process on the same GPU:
  pass_ms        dbgsom_covariance_apply at p = 8 with the true mean (both kernels: partials and their sum)
  colsums_ms     dbgsom_weighted_column_sums with unit weights on the same buffers: one pass over all columns, the
                 stream side.  pass and colsums are timed in turns, the order swapped every step.
  l1_lanes_per_s the float64 vector-instruction lanes per second dbgsom_bmu_manhattan reaches in this process on 2e5 x 784
                 rows against 1024 prototypes (tools/bench_manhattan.py's first shape: two lanes per pair and feature);
                 arithmetic_ms = 2 p N d fused multiply-adds (4 p N d flop) at that rate: the arithmetic side
  bound_ms       1.1 x the larger of the two; within_bound; side: the larger one ("stream" / "arithmetic"); a line that
                 misses says in "miss" where the time goes
  start_ms, start_passes   linear_init.principal_plane on the resident rows, host clock (the pass for the mean included
                 in the time, not in the count); start_residual: max_j |r_j| / theta_1 at the last pass
  fit_ms_pca / fit_ms_random   a whole SomVQ.fit with the parameters of bench.py's `fit` line and init="pca" (2 x 2 start) /
                 the default start; start_share = the time inside _start_prototypes over fit_ms_pca
  eigh_host_ms   the host alternative for scale: the float64 covariance of the same rows formed in chunks with BLAS, and
                 np.linalg.eigh of it; direction_err: |u - e| of init_directions_ against its two leading eigenvectors
                 (signs fixed alike), eigh_gap_ratio: l_1 / gap_j, what Davis-Kahan multiplies a residual by"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 784), (100_000, 64)]
L1_SHAPE = (200_000, 784, 1024)
P = 8
FIT_KW = dict(random_state=0, max_neurons=1024, n_iter=120, spreading_factor=0.9, convergence_iter=1,
              coarse_training_frac=0.7)
def miss(side, ratio, N, d, pass_ms):
    """Where a line that misses its bound spends its time, from the launch geometry of covariance.hip (512 workgroups at
    the most, at least 64 rows each, 4 rows per step, thread t of 256 owns the columns t, t + 256, ...)."""
    share = max(64, -(-(-(-N // 512)) // 4) * 4)
    steps = share // 4
    return (f"on the {side} side, {ratio} x its yardstick: a workgroup walks {steps} steps of 4 rows at "
            f"{pass_ms * 1e3 / steps:.1f} us each, {min(d, 256)} of its 256 threads own a column at d = {d}, and a step is "
            "one dependent chain (load, first product, fold of the 32 partial sums, two workgroup barriers, second "
            "product) with little to overlap it; not profiled further")


def med(t):
    return round(float(np.median(t)), 4), [round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--no-eigh", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_init_bench.json"))
    a = ap.parse_args()
    import torch

    import bench
    from dbgsom_amd import SomVQ, _native, linear_init
    from dbgsom_amd.backend import HipBackend

    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_init.py measures on the MI355X: no GPU visible")
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    F32 = _native.F32

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn):
        return med([one(fn) for _ in range(a.warmup + a.steps)][a.warmup:])

    def timed_in_turns(fa, fb):
        ta, tb = [], []
        for i in range(a.warmup + a.steps):
            if i % 2 == 0:
                ta.append(one(fa)), tb.append(one(fb))
            else:
                tb.append(one(fb)), ta.append(one(fa))
        return med(ta[a.warmup:]), med(tb[a.warmup:])

    def ws_of(nbytes):
        return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev), int(nbytes)

    # the arithmetic yardstick: the L1 search's float64 vector rate on this GPU, in this process
    Nl, dl, Ml = L1_SHAPE
    Xl = bench.make_shard(torch, Nl, dl, 1, dev)
    Wl = (Xl[:Ml].double() + 0.05 * torch.randn(Ml, dl, device=dev, dtype=torch.float64)).contiguous()
    idx = torch.empty(Nl, dtype=torch.int64, device=dev)
    dist = torch.empty(Nl, dtype=torch.float64, device=dev)
    ws, nb = ws_of(lib.dbgsom_bmu_manhattan_workspace_bytes(F32, Nl, dl, Ml))
    l1 = timed(lambda: _native.call("dbgsom_bmu_manhattan", Xl.data_ptr(), F32, Nl, dl, dl, Wl.data_ptr(), Ml, dl, 1,
                                    idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), nb, stream))
    l1_lanes = 2.0 * Nl * Ml * dl / (l1[0] * 1e-3)
    del Xl, Wl, idx, dist, ws
    torch.cuda.empty_cache()

    lines = []
    for si in (int(s) for s in a.shapes.split(",")):
        N, d = SHAPES[si]
        Xt = bench.make_shard(torch, N, d, bench.WORKLOADS["c4"][4], dev)
        mean = Xt.double().mean(dim=0).contiguous() if N * d < 10 ** 8 else \
            torch.stack([Xt[s:s + 100_000].double().sum(dim=0) for s in range(0, N, 100_000)]).sum(dim=0).div_(N).contiguous()
        V = torch.from_numpy(np.linalg.qr(np.random.default_rng(0).normal(size=(d, P)))[0].copy()).to(dev)
        Z = torch.empty((d, P), dtype=torch.float64, device=dev)
        cs = torch.empty(d, dtype=torch.float64, device=dev)
        wsc, nbc = ws_of(lib.dbgsom_covariance_apply_workspace_bytes(N, d, P))
        ones = torch.ones(N, dtype=torch.float64, device=dev)
        wcs = torch.empty(d, dtype=torch.float64, device=dev)
        wsw, nbw = ws_of(lib.dbgsom_weighted_column_sums_workspace_bytes(d))
        torch.cuda.synchronize()
        cov, col = timed_in_turns(
            lambda: _native.call("dbgsom_covariance_apply", Xt.data_ptr(), F32, N, d, d, mean.data_ptr(), V.data_ptr(), P,
                                 Z.data_ptr(), cs.data_ptr(), wsc.data_ptr(), nbc, stream),
            lambda: _native.call("dbgsom_weighted_column_sums", Xt.data_ptr(), F32, N, d, d, ones.data_ptr(), None,
                                 wcs.data_ptr(), wsw.data_ptr(), nbw, stream))
        del wsc, wsw, ones
        arithmetic_ms = round(2.0 * P * N * d / l1_lanes * 1e3, 4)
        yard = max(col[0], arithmetic_ms)
        bound = round(1.1 * yard, 4)
        rec = {"N": N, "d": d, "p": P, "dtype": "float32", "pass_ms": cov[0], "pass_ms_min_max": cov[1],
               "colsums_ms": col[0], "colsums_ms_min_max": col[1], "l1_ms": l1[0], "l1_shape": list(L1_SHAPE),
               "l1_lanes_per_s": round(l1_lanes, 1), "arithmetic_ms": arithmetic_ms, "bound_ms": bound,
               "within_bound": bool(cov[0] <= bound), "side": "stream" if col[0] >= arithmetic_ms else "arithmetic",
               "pass_over_stream": round(cov[0] / col[0], 3), "pass_over_arithmetic": round(cov[0] / arithmetic_ms, 3),
               "bytes_per_s": round(N * d * 4 / (cov[0] * 1e-3), 1), "flop_per_s": round(4.0 * P * N * d / (cov[0] * 1e-3), 1)}
        if not rec["within_bound"]:
            rec["miss"] = miss(rec["side"], round(cov[0] / yard, 2), N, d, cov[0])
        # the whole start on the resident rows
        be = HipBackend(0)
        be.load_device(Xt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plane = linear_init.principal_plane(be, N, d)
        rec.update({"start_ms": round((time.perf_counter() - t0) * 1e3, 2), "start_passes": int(plane.n_passes),
                    "start_residual": float(plane.residual), "start_cap": linear_init.MAX_PASSES})
        be.release()
        if not a.no_fit:
            for init in ("random", "pca"):
                est = SomVQ(init=init, **FIT_KW)
                inside = []
                orig = est._start_prototypes

                def spy(data, orig=orig, inside=inside):
                    t = time.perf_counter()
                    out = orig(data)
                    inside.append((time.perf_counter() - t) * 1e3)
                    return out

                est._start_prototypes = spy
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                est.fit(Xt)
                torch.cuda.synchronize()
                rec[f"fit_ms_{init}"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec[f"fit_neurons_{init}"], rec[f"fit_epochs_{init}"] = int(len(est.weights_)), int(est.n_iter_) + 1
                rec[f"fit_qe_{init}"] = float(est.quantization_error_)
                if init == "pca":
                    rec["start_in_fit_ms"] = round(inside[0], 2)
                    rec["start_share"] = round(inside[0] / rec["fit_ms_pca"], 4)
        if not a.no_eigh:
            t0 = time.perf_counter()
            mh = mean.cpu().numpy()
            cov64 = np.zeros((d, d))
            for s in range(0, N, 100_000):
                C = Xt[s:s + 100_000].cpu().numpy().astype(np.float64) - mh[None, :]
                cov64 += C.T @ C
            lam, E = np.linalg.eigh(cov64 / N)
            rec["eigh_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            lam, E = lam[::-1], E[:, ::-1].T
            errs, gaps = [], []
            for j in range(2):
                e = linear_init.fix_sign(E[j])
                errs.append(float(np.linalg.norm(plane.directions[j] - e)))
                gaps.append(float(lam[0] / np.abs(np.delete(lam, j) - lam[j]).min()))
            rec.update({"direction_err": errs, "eigh_gap_ratio": gaps, "variances": [float(v) for v in plane.variances],
                        "eigh_variances": [float(lam[0]), float(lam[1])], "eigh_ninth_variance": float(lam[min(8, d - 1)])})
        rec.update({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del Xt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
