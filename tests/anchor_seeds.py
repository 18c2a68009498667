"""Tables and references of the tests of the anchor seeds (csrc/filter.hip 2e, csrc/anchor_chain.h, engine.hip
ensure_anchors): tests/test_anchor_seeds_cpu.py, tests/test_gpu_anchor_seed_device.py.

Any seed keeps the filtered search exact, so bit-for-bit results say nothing about the seeds.  What is held to a
reference here is what the seed machinery itself leaves behind: the prototype anchor_seed_kernel chose per anchor
(against an np.longdouble arg-min with a derived rounding bound), the seed every sample got from its anchor, the
order of the anchor rows (against a NumPy restatement of the chain) and the bucket every sample went to (against the
emulation of the one-product pre-pass of tests/test_filter_bound.py)."""
import os
import shutil
import subprocess
import zlib

import numpy as np

import bench
from tests import test_filter_bound as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.longdouble
U = 2.0 ** -53
ANCHOR_MAX = 256
PRUNE, PRUNE_RETRY, SEED_FULL = 0x200, 0x800, 0x100


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- the chain (csrc/anchor_chain.h) ---------------------------------------------------------------------------------
def anchor_rows(N, A):
    return (np.arange(A, dtype=np.int64) * N) // A


def chain(anchors):
    """chain_anchors restated: squared distances summed feature by feature in float64 (the order of the C loop, no
    fused multiply-add), from row 0 to the nearest row not yet taken, ties (and distances that are not numbers) to
    the lower row -> the permutation"""
    a = np.asarray(anchors, dtype=np.float64)
    A, d = a.shape
    D = np.zeros((A, A))
    for k in range(d):
        t = a[:, None, k] - a[None, :, k]
        D += t * t
    taken = np.zeros(A, dtype=bool)
    out, cur = [], 0
    for _ in range(A):
        taken[cur] = True
        out.append(cur)
        best = -1
        row = D[cur]
        free = np.flatnonzero(~taken)
        if free.size:
            best = int(free[0])
            for j in free[1:]:
                if row[j] < row[best]:
                    best = int(j)
        cur = best
    return np.array(out, dtype=np.int64)


CHAIN_A = (3, 16, 256)
CHAIN_D = (16, 320)
CHAIN_INPUTS = ("blobs", "duplicates", "identical", "collinear")


def chain_input(name, A, d):
    """-> (A x d float64 rows, the chain known in advance or None)"""
    rng = _rng("chain", name, A, d)
    if name == "blobs":
        return bench.make_shard_numpy(A, d, 500 + A + d).astype(np.float64), None
    if name == "duplicates":                     # every row occurs twice or more: exact ties at distance 0 and beyond
        base = rng.standard_normal(((A + 2) // 3, d))
        return np.ascontiguousarray(base[rng.integers(0, base.shape[0], A)]), None
    if name == "identical":                      # every distance 0: the chain is 0, 1, 2, ...
        return np.tile(rng.standard_normal((1, d)), (A, 1)), np.arange(A, dtype=np.int64)
    if name == "collinear":
        # Row k at position pos[k] on a line (small integers times a direction of powers of two: every distance is
        # exact).  Row 0 at 0, one row at -3, the others at 3, 6, 9, ... in shuffled order.  From 0 the rows at +3 and
        # -3 tie and the lower row wins.  From +3 the row at +6 is nearer than the one at -3, so the chain walks
        # outwards and takes -3 last; from -3 the nearest free row is the one at +3, and outwards from there.
        pos = np.zeros(A)
        pos[1:] = 3.0 * (1 + rng.permutation(A - 1))
        far, near = int(np.argmax(pos)), int(np.flatnonzero(pos == 3.0)[0])
        if (near < far) != (d == 16):            # (d = 16: the row at +3 is the lower one; otherwise the row at -3)
            pos[far], pos[near] = pos[near], pos[far]
            far, near = near, far
        pos[far] = -3.0
        direction = np.zeros(d)
        direction[[0, d // 2, d - 1]] = (1.0, -0.5, 0.25)
        X = pos[:, None] * direction[None, :]
        rest = [int(k) for k in np.argsort(pos) if pos[k] > 3.0]
        known = [0, near] + rest + [far] if near < far else [0, far, near] + rest
        return X, np.array(known, dtype=np.int64)
    raise KeyError(name)


def run_chain_check(cases, workdir, sanitize=False):
    """tests/anchor_chain_check.cpp (host C++ compiler) on `cases` = [(N, rows A x d)] -> per case (strided rows,
    chained rows)"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    exe = os.path.join(str(workdir), "anchor_chain_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "dbgsom_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "anchor_chain_check.cpp")], check=True)
    lines = []
    for N, a in cases:
        A, d = a.shape
        lines.append(f"{N} {A} {d}")
        lines += [" ".join(float(v).hex() for v in row) for row in a]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    got = [np.array(ln.split()[1:], dtype=np.int64) for ln in out.strip().splitlines()]
    assert len(got) == 2 * len(cases), out[-500:]
    return [(got[2 * k], got[2 * k + 1]) for k in range(len(cases))]


# ---- the arg-min of anchor_seed_kernel -------------------------------------------------------------------------------
def finite_rows(W):
    """rows the kernel may choose while one of them exists: finite, with a finite squared norm"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(W).all(axis=1) & np.isfinite((W * W).sum(axis=1))


def argmin_reference(anchors, W):
    """v[a, j] = |w_j|^2 - 2 a . w_j in np.longdouble and bound[a, j] = (d + 16) 2^-53 (|w_j|^2 + 2 sum_k |a_k w_jk|):
    at most d + 2 roundings of terms of this size on the way to the kernel's float64 value (d in the norm, d in the
    product -- twice that weight --, one in the difference); the shape of the `rounding` term of filter_eps.
    Rows that are not finite_rows() get v = +inf, bound 0.  -> (v, bound), A x M np.longdouble"""
    a = np.asarray(anchors, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    d = a.shape[1]
    fin = finite_rows(W)
    Wz = np.where(fin[:, None], W, 0.0)
    al, wl = a.astype(L), Wz.astype(L)
    ww = (wl * wl).sum(axis=1)
    v = np.empty((a.shape[0], W.shape[0]), dtype=L)
    bound = np.empty_like(v)
    for s in range(0, W.shape[0], 512):
        wt = np.ascontiguousarray(wl[s:s + 512].T)
        v[:, s:s + 512] = ww[None, s:s + 512] - 2 * (al @ wt)
        bound[:, s:s + 512] = L(d + 16) * L(U) * (ww[None, s:s + 512] + 2 * (np.abs(al) @ np.abs(wt)))
    v[:, ~fin] = np.inf
    bound[:, ~fin] = 0
    return v, bound


def check_argmin(aseed, anchors, W, ref=None, tied=()):
    """the checks of an `aseed` against argmin_reference: in range; v[a, aseed[a]] <= min_j v + 2 max_j bound; equal to
    the reference arg-min where its runner-up is more than 2 max bound away; no anchor ambiguous outside `tied`
    (anchors whose minimum is a constructed tie: there only the first check applies and the caller asserts the
    index).  With no finite row: aseed == 0.  -> number of anchors checked for equality"""
    aseed = np.asarray(aseed)
    A, M = anchors.shape[0], W.shape[0]
    assert aseed.shape == (A,) and (aseed >= 0).all() and (aseed < M).all(), "a seed outside [0, M)"
    if not finite_rows(W).any():
        assert not aseed.any(), "no finite prototype: every key is +inf and the lowest index, 0, wins"
        return 0
    v, bound = ref if ref is not None else argmin_reference(anchors, W)
    vmin, slack = v.min(axis=1), 2 * bound.max(axis=1)
    rows = np.arange(A)
    assert finite_rows(W)[aseed].all(), "a non-finite prototype was chosen while a finite one exists"
    assert (v[rows, aseed] <= vmin + slack).all(), "a seed that is not a nearest prototype of its anchor"
    if M == 1:
        return A
    runner = np.partition(v, 1, axis=1)[:, 1]
    clear = runner - vmin > slack
    clear_free = clear.copy()
    clear_free[list(tied)] = True
    assert clear_free.all(), f"{int((~clear_free).sum())} ambiguous anchors: the case does not test the arg-min"
    eq = clear.copy()
    eq[list(tied)] = False
    assert np.array_equal(aseed[eq], v.argmin(axis=1)[eq]), "not the arg-min where the runner-up is clear"
    return int(eq.sum())


# ---- dbgsom_bmu_filtered_anchored called raw --------------------------------------------------------------------------
SEED_A = (1, 15, 16, 17, 255, 256)
SEED_M = (1, 15, 16, 17, 63, 64, 65, 130, 1985, 8192)     # the 16-prototype tile, the 64-prototype block; 1985, 8192: more
SEED_D = (16, 48, 64, 320)                                 # than 16 blocks, so the last workgroup's loop strides
SEED_KINDS = ("blobs", "iso")
SEED_DTYPES = ("f32", "f64")
SEED_BUCKETS = ("nearest", "random", "zeros", "last")
SEED_N = 300
# (A, M, d, kind, dtype, anchor_of): every pair of values of every two columns occurs in a row, but M = 8192 comes
# at d = 16 only (tests/test_anchor_seeds_cpu.py checks that)
SEED_CASES = (
    (16, 17, 48, 'blobs', 'f32', 'zeros'),
    (17, 130, 16, 'blobs', 'f64', 'nearest'),
    (16, 15, 64, 'iso', 'f64', 'last'),
    (256, 130, 320, 'iso', 'f32', 'random'),
    (255, 63, 64, 'blobs', 'f32', 'nearest'),
    (15, 1985, 320, 'blobs', 'f64', 'zeros'),
    (1, 64, 48, 'blobs', 'f64', 'random'),
    (1, 1985, 16, 'iso', 'f32', 'last'),
    (15, 1, 48, 'iso', 'f32', 'nearest'),
    (255, 65, 16, 'iso', 'f64', 'zeros'),
    (256, 16, 48, 'blobs', 'f64', 'last'),
    (17, 64, 320, 'iso', 'f32', 'last'),
    (15, 8192, 16, 'blobs', 'f64', 'random'),
    (16, 65, 320, 'blobs', 'f32', 'nearest'),
    (17, 17, 64, 'iso', 'f64', 'random'),
    (1, 1, 64, 'blobs', 'f64', 'zeros'),
    (16, 63, 16, 'iso', 'f64', 'random'),
    (1, 16, 320, 'iso', 'f32', 'nearest'),
    (255, 15, 320, 'blobs', 'f32', 'random'),
    (256, 8192, 16, 'iso', 'f32', 'nearest'),
    (255, 130, 48, 'iso', 'f32', 'last'),
    (17, 63, 48, 'iso', 'f32', 'zeros'),
    (15, 65, 64, 'iso', 'f64', 'last'),
    (256, 64, 64, 'blobs', 'f64', 'zeros'),
    (17, 16, 16, 'iso', 'f64', 'zeros'),
    (256, 1, 320, 'iso', 'f64', 'random'),
    (1, 17, 16, 'blobs', 'f64', 'nearest'),
    (1, 15, 48, 'blobs', 'f64', 'zeros'),
    (16, 1985, 64, 'blobs', 'f32', 'random'),
    (255, 1985, 48, 'iso', 'f64', 'nearest'),
    (256, 15, 16, 'blobs', 'f32', 'nearest'),
    (16, 16, 64, 'blobs', 'f64', 'random'),
    (1, 65, 48, 'blobs', 'f64', 'random'),
    (17, 1, 16, 'blobs', 'f32', 'last'),
    (15, 130, 64, 'iso', 'f32', 'zeros'),
    (15, 63, 320, 'iso', 'f64', 'last'),
    (255, 17, 320, 'blobs', 'f64', 'last'),
    (255, 64, 16, 'iso', 'f32', 'nearest'),
    (16, 8192, 16, 'blobs', 'f32', 'last'),
    (255, 8192, 16, 'blobs', 'f32', 'zeros'),
    (16, 64, 16, 'blobs', 'f64', 'nearest'),
    (256, 1985, 320, 'blobs', 'f64', 'zeros'),
    (17, 15, 64, 'iso', 'f64', 'nearest'),
    (15, 15, 64, 'blobs', 'f32', 'nearest'),
    (15, 17, 16, 'iso', 'f32', 'last'),
    (1, 130, 16, 'blobs', 'f32', 'last'),
    (1, 63, 48, 'blobs', 'f64', 'random'),
    (17, 65, 48, 'iso', 'f32', 'random'),
    (16, 130, 64, 'blobs', 'f64', 'nearest'),
    (256, 63, 48, 'iso', 'f64', 'zeros'),
    (255, 1, 48, 'blobs', 'f64', 'nearest'),
    (256, 65, 16, 'blobs', 'f64', 'last'),
    (15, 16, 320, 'blobs', 'f32', 'zeros'),
    (17, 1985, 48, 'blobs', 'f64', 'zeros'),
    (256, 17, 64, 'iso', 'f64', 'random'),
    (16, 1, 48, 'iso', 'f32', 'random'),
    (15, 64, 64, 'iso', 'f32', 'random'),
    (255, 16, 48, 'blobs', 'f64', 'nearest'),
    (17, 8192, 16, 'blobs', 'f32', 'nearest'),
    (1, 8192, 16, 'blobs', 'f64', 'last'),
)
# beyond the pairs, (N, flags, case): one sample set of 129 rows (two workgroups, the second of one sample) and one
# call with the re-seeding passes, which overwrite seeds: there only the arg-min and the search results are checked
SEED_EXTRA = (
    (129, PRUNE, (17, 65, 48, 'blobs', 'f32', 'nearest')),
    (SEED_N, PRUNE | PRUNE_RETRY, (256, 130, 64, 'blobs', 'f32', 'nearest')),
)
SEED_ROWS = tuple((SEED_N, PRUNE, c) for c in SEED_CASES) + SEED_EXTRA


def seed_row_id(row):
    N, flags, c = row
    return "-".join(map(str, c)) + (f"-N{N}" if N != SEED_N else "") + ("-retry" if flags & PRUNE_RETRY else "")


def nearest_anchor(X, anchors):
    """the exact nearest anchor of every row (np.longdouble, ties to the lower anchor)"""
    return fb_exact_r(X, anchors).argmin(axis=1).astype(np.int32)


def fb_exact_r(X, W):
    Xl, Wl = np.asarray(X, dtype=np.float64).astype(L), np.asarray(W, dtype=np.float64).astype(L)
    return (Xl ** 2).sum(1)[:, None] - 2 * (Xl @ np.ascontiguousarray(Wl.T)) + (Wl ** 2).sum(1)[None, :]


def seed_inputs(row):
    """-> dict: X (N x d as stored), W (M x d float64: sample rows plus 0.05 noise), anchors (A x d float64: the
    strided rows of X, in chain order where there are more than two), anchor_of (int32), order (its stable argsort)"""
    N, flags, (A, M, d, kind, dtype, buckets) = row
    X = bench.make_shard_numpy(N, d, 1000 + N + d + M, kind=kind)
    if dtype == "f64":                                   # (float64 rows that are no float32 values)
        X = X.astype(np.float64) * (1.0 + 2.0 ** -30)
    rng = _rng("seed", row)
    W = X[rng.choice(N, M, replace=M > N)].astype(np.float64) + 0.05 * rng.standard_normal((M, d))
    anchors = np.ascontiguousarray(X[anchor_rows(N, A)], dtype=np.float64)
    if A > 2:
        anchors = np.ascontiguousarray(anchors[chain(anchors)])
    if buckets == "nearest":
        anchor_of = nearest_anchor(X, anchors)
    elif buckets == "random":
        anchor_of = rng.integers(0, A, N).astype(np.int32)
    elif buckets == "zeros":
        anchor_of = np.zeros(N, dtype=np.int32)
    elif buckets == "last":
        anchor_of = np.full(N, A - 1, dtype=np.int32)
    else:
        raise KeyError(buckets)
    return {"X": X, "W": np.ascontiguousarray(W), "anchors": anchors, "anchor_of": anchor_of,
            "order": np.argsort(anchor_of, kind="stable").astype(np.int32)}


# ties: bit-identical copies of one prototype row; one anchor equals them, so they are its nearest prototypes by far
# and the lowest index must win.  In M = 200 prototype j is block j / 64, wavefront (j % 64) / 16, and within the
# wavefront's 16 x 16 tile accumulator slot (j % 16) / 4 of lane group j % 4; at M = 1985 block p is reduced by thread
# p % 16 of the last workgroup in round p / 16.
TIE_SETS = (
    (200, 48, (70, 134)),            # another 64-block
    (200, 48, (70, 86)),             # another wavefront of the block
    (200, 48, (70, 74)),             # another accumulator slot of the same lanes
    (200, 48, (70, 71)),             # the next lane group, same slot
    (200, 48, (74, 86, 134, 199)),   # all of them, the lowest in a later slot
    (200, 48, (0, 199)),
    (1985, 16, (70, 1094)),          # blocks 1 and 17: the same thread of the last workgroup, two rounds
    (1985, 16, (1100, 1900)),        # blocks 17 and 29, second round only
    (1985, 16, (1023, 1024, 1984)),  # across the end of the first round, and the last prototype
)
TIE_A, TIE_ANCHOR = 17, 16           # the tied anchor is the only one of the second anchor block


def tie_inputs(case):
    M, d, copies = case
    row = (SEED_N, PRUNE, (TIE_A, M, d, "blobs", "f32", "nearest"))
    inp = seed_inputs(row)
    W = inp["W"]
    W[list(copies)] = W[copies[-1]]                      # (the copy with the highest index is the original)
    inp["anchors"][TIE_ANCHOR] = W[copies[0]]
    inp["anchor_of"] = nearest_anchor(inp["X"], inp["anchors"])
    inp["order"] = np.argsort(inp["anchor_of"], kind="stable").astype(np.int32)
    return inp


BAD_KINDS = ("nan", "inf", "overflow")


def bad_row(kind, d):
    r = np.full(d, 0.5)
    if kind == "nan":
        r[d // 2] = np.nan
    elif kind == "inf":
        r[3] = -np.inf
    elif kind == "overflow":                             # finite entries, |w|^2 = +inf
        r[:] = 1e200
    else:
        raise KeyError(kind)
    return r


def bad_inputs(M, d, every_row):
    """a map with a NaN row, a row with an infinity and a finite row whose squared norm overflows -- at index 0, in
    the middle and at the end, or (every_row) nothing else"""
    inp = seed_inputs((SEED_N, PRUNE, (ANCHOR_MAX, M, d, "blobs", "f32", "nearest")))
    W = inp["W"]
    where = range(M) if every_row else (0, M // 2, M - 1)
    for n, j in enumerate(where):
        W[j] = bad_row(BAD_KINDS[n % 3], d)
    return inp


# ---- the context's buckets --------------------------------------------------------------------------------------------
CTX_N = (200, 256, 257, 1000, 4096)
CTX_D = 70                                               # padded to 80 on the device
CTX_STORAGE = ("float32", "float64", "bf16")
QUALITY_FACTOR, QUALITY_ABS = 1.5, 1e-4


def emulated_buckets(X, anchors):
    """the pre-pass that builds the buckets (every anchor, every feature, one digit product: DBGSOM_SEED_FULL with
    sweep_planes = 1) as tests/test_filter_bound.py emulates it -> (anchor_of, exact squared distances N x A in
    np.longdouble, eps_i of filter_eps(planes=1) with the anchors as the map)"""
    X = np.asarray(X, dtype=np.float64)
    rt, (sx, l1x, xx, tw, l1w, yy) = fb.r_tilde(X, anchors, levels=1)
    eps = fb.filter_eps(sx, l1x, xx, l1w.max(), tw.max(), yy.max(), X.shape[1], 1)
    return rt.argmin(axis=1), fb_exact_r(X, anchors), eps


def bucket_quality(r, anchor_of):
    """-> (summed distance to the assigned anchor / summed distance to the nearest anchor - 1, share of the samples
    at their exact nearest anchor)"""
    n = np.arange(r.shape[0])
    mine, best = r[n, anchor_of], r.min(axis=1)
    dist = lambda q: float(np.sqrt(np.maximum(q, 0)).sum())
    return dist(mine) / max(dist(best), 1e-300) - 1.0, float((mine == best).mean())


def check_buckets(anchor_of, order, r, eps, A):
    """what holds for the buckets whatever the rounding: in range, `order` the stable argsort, and the assigned
    anchor within 2 eps_i of the nearest"""
    N = r.shape[0]
    anchor_of, order = np.asarray(anchor_of), np.asarray(order)
    assert anchor_of.shape == (N,) and (anchor_of >= 0).all() and (anchor_of < A).all()
    assert np.array_equal(order, np.argsort(anchor_of, kind="stable")), "order is not the stable argsort of anchor_of"
    n = np.arange(N)
    assert (r[n, anchor_of] <= r.min(axis=1) + 2 * eps.astype(L)).all(), "a sample beyond 2 eps of its nearest anchor"
