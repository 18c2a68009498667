"""The topographic function on the MI355X (csrc/topofn.hip): one JSON line per shape.

    python tools/bench_topofn.py [--shapes c4,c5map,m16k] [--host-rows N]

Each line: the whole call of HipBackend.topographic_function in histogram mode (upload of X, the k = 2
search, the graph stage) and its stage split from a second, timed call (HIP events: search, edge set +
CSR + lattice neighbours, distances, histograms); the same for full mode (the M x M hop distances copied
back); the graph's ordered edges and diameter; and the host default (scikit-learn's 2-NN search on the
first --host-rows rows + scipy's unweighted shortest paths) on the same map, with the device's result on
those rows for comparison.  Shapes:
    c4     bench.py's generator, N = 1e6, d = 784 (float32), a 32 x 32 map
    c5map  a 64 x 64 map (C5's size), 2e5 float32 rows of d = 2048
    m16k   M = 16 000 (125 x 128), 2e5 float32 rows of d = 64
Maps: c4 prototypes are the mean of the rows in each cell of a quantile grid over the data's first two
principal axes (a random row in an empty cell); c5map / m16k prototypes sit on a jittered grid of a 2-D
sheet in d dimensions that the rows sample, as the tests' maps do."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c4": (1_000_000, 784, 32, 32), "c5map": (200_000, 2048, 64, 64), "m16k": (200_000, 64, 125, 128)}
# estimates of the issue that asked for this, not measurements: graph stage (edges -> histograms), whole call
TARGETS = {"c4": {"graph_ms": 2.0, "call_s": 0.5}, "c5map": {"graph_ms": 10.0}, "m16k": {"graph_ms": 50.0}}


def pca_grid_map(X, rows, cols, seed):
    """Prototypes = the mean of the rows in each cell of a rows x cols quantile grid over the first two
    principal axes (an empty cell takes a random row: no two prototypes alike)."""
    rng = np.random.default_rng(seed)
    sub = X[rng.choice(len(X), min(len(X), 20000), replace=False)].astype(np.float64)
    mu = sub.mean(axis=0)
    _, _, vt = np.linalg.svd(sub - mu, full_matrices=False)
    Z = (X @ vt[:2].T.astype(np.float32)) - (mu @ vt[:2].T).astype(np.float32)
    qi = np.quantile(Z[:, 0], np.linspace(0, 1, rows + 1)[1:-1])
    qj = np.quantile(Z[:, 1], np.linspace(0, 1, cols + 1)[1:-1])
    cell = np.searchsorted(qi, Z[:, 0]) * cols + np.searchsorted(qj, Z[:, 1])
    cnt = np.bincount(cell, minlength=rows * cols).astype(np.float64)
    from scipy.sparse import csr_matrix

    W = np.asarray(csr_matrix((np.ones(len(X)), (cell, np.arange(len(X)))), shape=(rows * cols, len(X))) @ X,
                   dtype=np.float64)
    full = cnt > 0
    W[full] /= cnt[full, None]
    empty = np.flatnonzero(~full)
    W[empty] = X[rng.choice(len(X), len(empty), replace=False)]
    ii, jj = np.divmod(np.arange(rows * cols), cols)
    return W, np.c_[ii, jj]


def sheet_map(n, d, rows, cols, seed):
    rng = np.random.default_rng(seed)
    ii, jj = np.divmod(np.arange(rows * cols), cols)
    P = rng.normal(size=(2, d)).astype(np.float32)
    W = (np.c_[ii, jj] + rng.uniform(-0.2, 0.2, size=(rows * cols, 2))) @ P.astype(np.float64)
    X = np.empty((n, d), dtype=np.float32)
    for s in range(0, n, 50000):
        m = min(50000, n - s)
        S = rng.uniform(-0.5, [rows - 0.5, cols - 0.5], size=(m, 2)).astype(np.float32)
        X[s:s + m] = S @ P + rng.normal(0, 0.01, size=(m, d)).astype(np.float32)
    return W, X, np.c_[ii, jj]


class HostSearch:
    """The host default of HotPathBackend.topographic_function with scikit-learn's 2-NN search (the
    reference's _get_winning_neurons)."""

    def __new__(cls):
        from dbgsom_amd.backend import HotPathBackend

        class _H(HotPathBackend):
            def bmu(self, W, k=1, X=None):
                from sklearn.neighbors import NearestNeighbors

                nn = NearestNeighbors(n_neighbors=k, n_jobs=16).fit(W)
                dist, idx = nn.kneighbors(X)
                return dist, idx

        return _H()


def timed_call(hip, lib, W, X, xy, full):
    lib.dbgsom_topofn_timing(1)
    t0 = time.perf_counter()
    out = hip.topographic_function(W, X, xy, want_distances=full)
    t = time.perf_counter() - t0
    ms = (ctypes.c_double * 4)()
    lib.dbgsom_topofn_stage_ms(ms)
    lib.dbgsom_topofn_timing(0)
    ms = [round(float(v), 3) for v in ms]
    return out, t, {"search_ms": ms[0], "edges_csr_ms": ms[1], "distances_ms": ms[2], "histograms_ms": ms[3],
                    "graph_ms": round(ms[1] + ms[2] + ms[3], 3), "timed_call_s": round(t, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,c5map,m16k")
    ap.add_argument("--host-rows", type=int, default=20000)
    a = ap.parse_args()
    import bench
    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    lib = _native.load()
    hip = HipBackend(0)
    for name in a.shapes.split(","):
        N, d, rows, cols = SHAPES[name]
        if name == "c4":
            X = bench.make_shard_numpy(N, d, 0)
            W, xy = pca_grid_map(X, rows, cols, 1)
        else:
            W, X, xy = sheet_map(N, d, rows, cols, 2)
        M = rows * cols
        hip.topographic_function(W, X[:1000], xy)  # warm-up (module load, first allocations)
        t0 = time.perf_counter()
        hp, hn, _ = hip.topographic_function(W, X, xy)
        t_call = time.perf_counter() - t0
        _, _, st = timed_call(hip, lib, W, X, xy, False)
        t0 = time.perf_counter()
        fp, fn, D = hip.topographic_function(W, X, xy, want_distances=True)
        t_full = time.perf_counter() - t0
        _, _, st_full = timed_call(hip, lib, W, X, xy, True)
        line = {"shape": name, "N": N, "d": d, "M": M, "lattice": [rows, cols],
                "call_s": round(t_call, 4), "stages": st,
                "full_call_s": round(t_full, 4), "full_stages": st_full,
                "modes_agree": bool(np.array_equal(hp, fp) and np.array_equal(hn, fn)),
                "edges_ordered": int(hp.sum()), "diameter": int(D.max()),
                "unreachable_pairs": int((D < 0).sum()), "lattice_pairs_ordered": int(hn.sum())}
        del D
        if M <= 4096:
            nh = min(N, a.host_rows)
            Xh = X[:nh]
            host = HostSearch()
            t0 = time.perf_counter()
            rp, rn, _ = host.topographic_function(W, Xh, xy)
            t_host = time.perf_counter() - t0
            dp, dn, _ = hip.topographic_function(W, Xh, xy)
            line["host"] = {"rows": nh, "s": round(t_host, 3), "equal_to_device": bool(
                np.array_equal(rp, dp) and np.array_equal(rn, dn))}
        tg = TARGETS[name]
        line["targets"] = dict(tg, met=bool(st["graph_ms"] <= tg["graph_ms"]
                                            and ("call_s" not in tg or t_call <= tg["call_s"])))
        print(json.dumps(line), flush=True)
    hip.release()


if __name__ == "__main__":
    main()
