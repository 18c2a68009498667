"""Device tensors against host arrays as the X of the estimators on the MI355X: one JSON line per workload, also
written to --out (default profiles/device_input_bench.json).

    python tools/bench_device_input.py [--workloads predict,qe,transform,predict_proba,fit] [--steps 10] [--warmup 2]
                                       [--rows N] [--code-rows N]

Workloads (float32 rows generated in HBM as bench.py generates workload c4, d = 784; the host array is their copy):
  predict, qe            SomVQ.predict / calculate_quantization_error of 1e6 rows on a map of M = 1024 prototypes
                         (planted into a fitted SomVQ: rows of X plus noise -- a fit leaves fewer than it grew)
  transform              SomVQ.transform of 1e5 rows on the same map
  predict_proba          SomClassifier.predict_proba of 1e5 rows on a map fitted to 32 classes of the first 2e5 rows
  fit                    a whole SomVQ.fit with the parameters of bench.py's `fit` line
Each line:
  tensor_ms / host_ms    host clock around the blocking call, X a tensor on the GPU / the same rows as a host array
                         (the host-array path is the code as it was before tensors were accepted); median of --steps
                         after --warmup, with [min, max]
  device_ms              the device time inside: predict / qe -- row norms, digit planes and the stateless filtered
                         search as the context runs them for a query of this size, HIP events on one stream around
                         the device-level calls on the rows in HBM; transform / predict_proba -- the summed stage
                         times of the coder (dbgsom_sparse_code_stage_ms) over one tensor call; fit -- none
  x_upload_bytes, x_download_bytes   the context's sample-traffic counters over ONE call of each path
  host_upload_bytes_per_s, host_download_bytes_per_s   what the host path's extra time buys: its counters over
                         (host_ms - tensor_ms); null where the host path is not the slower one
  equal                  the two paths' results are the same bits"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, M_PLANTED = 784, 1024
FIT_KW = dict(random_state=0, max_neurons=1024, n_iter=120, spreading_factor=0.9, convergence_iter=1,
              coarse_training_frac=0.7)


def stats(fn, steps, warmup):
    t = []
    for _ in range(warmup + steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t = t[warmup:]
    return round(float(np.median(t)), 3), [round(float(np.min(t)), 3), round(float(np.max(t)), 3)]


def traffic_of(be, fn):
    before = be.sample_traffic()
    out = fn()
    after = be.sample_traffic()
    return out, {k: after[k] - before[k] for k in ("x_upload_bytes", "x_download_bytes")}


def same_bits(a, b):
    if isinstance(a, float):
        return a == b
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="predict,qe,transform,predict_proba,fit")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--code-rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_input_bench.json"))
    a = ap.parse_args()
    import torch

    import bench
    from dbgsom_amd import SomClassifier, SomVQ, _native

    if not torch.cuda.is_available():
        raise SystemExit("bench_device_input.py measures on the MI355X: no GPU visible")
    dev = torch.device("cuda", 0)
    n, nc = a.rows, min(a.code_rows, a.rows)
    Xt = bench.make_shard(torch, n, D, bench.WORKLOADS["c4"][4], dev)
    Xh = Xt.cpu().numpy()
    rng = np.random.default_rng(0)
    wanted = a.workloads.split(",")
    lines = []

    def line(name, est, call, rows_t, rows_h, device_ms):
        be = est._engine()
        out_t, tr_t = traffic_of(be, lambda: call(rows_t))
        out_h, tr_h = traffic_of(be, lambda: call(rows_h))
        t_ms, t_mm = stats(lambda: call(rows_t), a.steps, a.warmup)
        h_ms, h_mm = stats(lambda: call(rows_h), a.steps, a.warmup)
        extra = (h_ms - t_ms) * 1e-3
        rec = {"workload": name, "N": int(rows_h.shape[0]), "d": D, "M": len(est.neurons_) if name == "predict_proba"
               else int(est.weights_.shape[0]), "dtype": "float32",
               "tensor_ms": t_ms, "tensor_ms_min_max": t_mm, "host_ms": h_ms, "host_ms_min_max": h_mm,
               "device_ms": device_ms, "tensor": tr_t, "host": tr_h,
               "host_upload_bytes_per_s": round(tr_h["x_upload_bytes"] / extra) if extra > 0 else None,
               "host_download_bytes_per_s": round(tr_h["x_download_bytes"] / extra)
               if extra > 0 and tr_h["x_download_bytes"] else None,
               "equal": bool(same_bits(out_t, out_h)), "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    if {"predict", "qe", "transform"} & set(wanted):
        vq = SomVQ(random_state=0, n_iter=8).fit(Xt[:4096])
        W = Xh[rng.choice(n, M_PLANTED, replace=False)].astype(np.float64) + 0.05 * rng.standard_normal((M_PLANTED, D))
        vq.weights_ = W          # (predict, the error and the code read nothing else of the map)
        if {"predict", "qe"} & set(wanted):
            search_ms = search_device_ms(torch, _native, Xt, W, a.steps, a.warmup)
            if "predict" in wanted:
                line("predict", vq, vq.predict, Xt, Xh, search_ms)
            if "qe" in wanted:
                line("qe", vq, vq.calculate_quantization_error, Xt, Xh, search_ms)
        if "transform" in wanted:
            line("transform", vq, vq.transform, Xt[:nc], Xh[:nc], coder_device_ms(_native, lambda: vq.transform(Xt[:nc])))
    if "predict_proba" in wanted:
        nf = min(n, 200_000)
        y = rng.integers(0, 32, nf)
        clf = SomClassifier(random_state=0, n_iter=30, max_neurons=256, spreading_factor=0.9).fit(Xt[:nf], y)
        line("predict_proba", clf, clf.predict_proba, Xt[:nc], Xh[:nc],
             coder_device_ms(_native, lambda: clf.predict_proba(Xt[:nc])))
    if "fit" in wanted:
        SomVQ(**dict(FIT_KW, n_iter=8)).fit(Xt[:4096])     # (library and allocator warm)
        est = SomVQ(**FIT_KW)

        def fit(rows):
            est.fit(rows)
            return est.weights_

        line("fit", est, fit, Xt, Xh, None)
        lines[-1]["epochs"] = int(est.n_iter_) + 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


def search_device_ms(torch, _native, Xt, W, steps, warmup):
    """Row norms, digit planes and the stateless filtered search (library defaults) on the rows in HBM, between two
    HIP events on the current torch stream."""
    lib = _native.load()
    n, d = Xt.shape
    M = W.shape[0]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Wt = torch.from_numpy(W).cuda()
    xx = torch.empty(n, dtype=torch.float64, device="cuda")
    ww = torch.empty(M, dtype=torch.float64, device="cuda")
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    dist = torch.empty(n, dtype=torch.float64, device="cuda")
    pbytes = lib.dbgsom_filter_planes_bytes(n, d)
    planes = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    wbytes = lib.dbgsom_bmu_filtered_workspace_bytes(n, d, M)
    ws = torch.zeros(wbytes, dtype=torch.uint8, device="cuda")

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _native.call("dbgsom_row_sqnorms", Xt.data_ptr(), _native.F32, n, d, d, xx.data_ptr(), stream)
        _native.call("dbgsom_row_sqnorms", Wt.data_ptr(), _native.F64, M, d, d, ww.data_ptr(), stream)
        _native.call("dbgsom_filter_prepare", Xt.data_ptr(), _native.F32, n, d, d, planes.data_ptr(), pbytes, stream)
        _native.call("dbgsom_bmu_filtered", Xt.data_ptr(), _native.F32, n, d, d, xx.data_ptr(), planes.data_ptr(),
                     Wt.data_ptr(), M, ww.data_ptr(), None, None, 0, 0, 0, idx.data_ptr(), dist.data_ptr(),
                     ws.data_ptr(), wbytes, stream)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    t = [once() for _ in range(warmup + steps)][warmup:]
    return round(float(np.median(t)), 3)


def coder_device_ms(_native, call):
    ms = (ctypes.c_double * 5)()
    _native.call("dbgsom_sparse_code_timing", 1)
    try:
        call()
        _native.call("dbgsom_sparse_code_stage_ms", ms)
    finally:
        _native.call("dbgsom_sparse_code_timing", 0)
    return round(float(sum(ms)), 3)


if __name__ == "__main__":
    main()
