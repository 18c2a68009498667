"""NumPy emulation of the candidate lists of the pruning form under two kinds of seeds, without the
kernels' rounding margins and without re-seeding passes: seeds from anchor buckets (256 strided rows of X numbered
along a nearest-neighbour chain, samples bucketed by nearest anchor, seed = the anchor's nearest prototype) against the
cheap pre-pass (every stride-th prototype on 192 features, samples bucketed by seed).  Prints the mean and the longest
list per 128-sample workgroup.    python tools/anchor_list_emulation.py [rows]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
def run(N, d, rows, cols, seed, kind="blobs"):
    M = rows*cols
    X = bench.make_shard_numpy(N, d, seed, kind)
    W = X[np.random.default_rng(seed + 7).choice(N, M, replace=False)].astype(np.float64)
    Xd = X.astype(np.float64)
    def d2(A, B): return (A*A).sum(1)[:,None] - 2*A@B.T + (B*B).sum(1)[None]
    gapW = np.sqrt(np.maximum(d2(W, W), 0))
    def lists(seed_of, order):
        out = []
        for g in range(0, N, 128):
            ii = order[g:g+128]
            p = seed_of[ii]
            r = np.sqrt(np.maximum(((Xd[ii]-W[p])**2).sum(1), 0))
            keep = np.zeros(M, bool)
            for pp in np.unique(p):
                T = 2*r[p == pp].max()
                keep |= gapW[pp] < T
            out.append(keep.sum())
        return np.array(out)
    # anchors
    A = 256
    ar = (np.arange(A) * N) // A
    anc = Xd[ar]
    D = d2(anc, anc); taken = np.zeros(A, bool); chain = []; cur = 0
    for n in range(A):
        taken[cur] = True; chain.append(cur)
        dd = np.where(taken, np.inf, D[cur]); cur = int(dd.argmin())
    anc = anc[chain]
    aof = d2(Xd, anc).argmin(1)
    order = np.argsort(aof, kind="stable")
    aseed = d2(anc, W).argmin(1)
    la = lists(aseed[aof], order)
    # pre-pass: every stride-th prototype, 192 features (first three tiles as a stand-in)
    stride = max(4, (M + 255)//256)
    sub = np.arange(0, M, stride)
    f = slice(0, 192)
    ps = sub[d2(Xd[:, f], W[sub][:, f]).argmin(1)]
    lp = lists(ps, np.argsort(ps, kind="stable"))
    print(f"N={N} d={d} M={M} {kind}: anchors mean {la.mean():.1f} max {la.max()}  pre-pass mean {lp.mean():.1f} max {lp.max()}  ratio {la.mean()/lp.mean():.2f}", flush=True)
run(ROWS, 784, 32, 32, 1004)          # C4's data and map, fewer rows
run(ROWS, 128, 45, 45, 1003)          # C3's
run(min(ROWS, 60_000), 784, 22, 23, 1002)   # C2
