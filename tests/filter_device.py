"""Helpers and case tables of the device-level tests of the filtered search (tests/test_gpu_filter_device.py,
tests/test_filter_device_cpu.py): dbgsom_filter_prepare, the gap table of the triangle-inequality form and
dbgsom_bmu_filtered called raw, the way include/dbgsom_hip.h allows and the context never does.

Staging is tests/device_abi.py's (NaN in the padding columns, element offsets, workspace()); the arithmetic the
kernels are held to is the emulation of tests/test_filter_bound.py (slice_rows, proto_gap, plane16's residual),
imported, not restated.  What is restated here are layouts and launcher forms: carve_planes (filter.hip) and, through
tests/filter_form_check.cpp, FilterForm::resolve (filter_form.h) -- so that the CPU file can check without a GPU that
the tables hold what they claim."""
import os
import shutil
import subprocess
import zlib

import numpy as np

from tests import device_abi as da
from tests import test_filter_bound as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_FULL, PRUNE, PRUNE_PROBE, PRUNE_RETRY, REFINE = 0x100, 0x200, 0x400, 0x800, 0x1000
FKT = 64                  # features per k-tile of a plane row (filter_form.h)
PRUNE_MAX_M = 8192        # largest map with a gap table
FILTER_MAX_M = 16000
L = np.longdouble


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- 1. the planes buffer of dbgsom_filter_prepare ------------------------------------------------------------------
def filter_dpad(d):
    p = (d + FKT - 1) // FKT * FKT
    return max(p, 2 * FKT)


def align256(n):
    return (n + 255) // 256 * 256


def planes_layout(rows, d):
    """carve_planes: int8 [3][rows][dpad], then scale, l1, res16 (float64 per row), each on a 256-byte boundary
    -> dict of byte offsets, 'dpad' and 'total'"""
    dpad = filter_dpad(d)
    o_scale = align256(3 * rows * dpad)
    o_l1 = o_scale + align256(8 * rows)
    o_res = o_l1 + align256(8 * rows)
    return {"dpad": dpad, "planes": 0, "scale": o_scale, "l1": o_l1, "res16": o_res, "total": o_res + align256(8 * rows)}


def split_planes(buf, rows, d):
    """the bytes of a planes buffer (uint8) -> (planes int8 [3, rows, dpad], scale, l1, res16)"""
    lay = planes_layout(rows, d)
    buf = np.ascontiguousarray(buf[:lay["total"]])
    planes = buf[:3 * rows * lay["dpad"]].view(np.int8).reshape(3, rows, lay["dpad"])
    f = lambda name: buf[lay[name]:lay[name] + 8 * rows].view(np.float64)
    return planes, f("scale"), f("l1"), f("res16")


PREP_ROWS = (1, 5, 131)                                # four rows per workgroup: one partial, two, 33 with a tail
PREP_D = (1, 16, 63, 64, 65, 128, 129, 200)            # dpad 128 / 192 / 256; lane loop with and without a tail
PREP_LAYOUTS = ((0, 0), (3, 0), (0, 1), (3, 1))        # (ld - d, base offset in elements)
PREP_DTYPES = ("f32", "f64", "bf16")
PREP_MAX = 2.5                                         # the +max / -max of the "extremes" row


def special_rows(d, rng):
    """-> [zeros, a row holding +max and -max, one huge and many tiny entries, small integers]"""
    ext = rng.uniform(-0.9, 0.9, d) * PREP_MAX
    ext[0] = PREP_MAX
    ext[d - 1] = -PREP_MAX if d > 1 else PREP_MAX
    huge = rng.normal(size=d) * 1e-6
    huge[d // 2] = 1e6
    ints = rng.integers(-4, 5, d).astype(np.float64)
    ints[0] = 4.0
    return [np.zeros(d), ext, huge, ints]


def prepare_rows(rows, d, dtype):
    """the rows of one dbgsom_filter_prepare case as stored for `dtype`: scaled normal rows; from five rows on, the
    special rows at 0 .. 3, from 131 on again in the last (partial) workgroup"""
    rng = _rng("prep", rows, d)
    A = rng.normal(size=(rows, d)) * rng.uniform(0.5, 3.0, size=d) * rng.uniform(0.1, 10.0, size=(rows, 1))
    if rows >= 5:
        A[:4] = special_rows(d, rng)
    if rows >= 131:
        A[rows - 4:] = special_rows(d, rng)[::-1]
    return da.stored(A, dtype)


def residual16(A):
    """|a - a16| per row in np.longdouble, a16 = s (256 D0 + D1) / F16 as plane16 forms it"""
    A = np.asarray(A, dtype=np.float64)
    (d0, d1, _), s, _ = fb.slice_rows(A)
    a16 = s.astype(L)[:, None] * (d0 * 256 + d1).astype(L) / L(fb.F16)
    return np.sqrt(((A.astype(L) - a16) ** 2).sum(axis=1))


def check_prepared(A, planes, scale, l1, res16, rows_to_check=None):
    """every check of issue section 1 on the finite rows of A (float64, as widened); -> the largest l1 error / bound
    and the largest res16 / |a - a16| over the rows with a non-zero residual"""
    A = np.asarray(A, dtype=np.float64)
    rows, d = A.shape
    sel = np.arange(rows) if rows_to_check is None else np.asarray(rows_to_check)
    (d0, d1, d2), s, _ = fb.slice_rows(A)
    dpad = planes.shape[2]
    assert dpad == filter_dpad(d)
    for got, want in zip(planes, (d0, d1, d2)):
        assert np.array_equal(got[sel, :d], want[sel]), "digit planes differ from slice_rows"
        assert not got[sel, d:].any(), "plane columns d .. dpad must be 0"
    assert np.array_equal(scale[sel], s[sel]), "row scales differ from slice_rows"
    T = np.abs(A.astype(L)).sum(axis=1)
    bound = (-(-d // 64) + 6) * da.U * T
    err = np.abs(l1.astype(L) - T)
    assert (err[sel] <= bound[sel]).all(), "l1 outside (ceil(d / 64) + 6) u sum |a_k|"
    res = residual16(A)
    amax = np.abs(A).max(axis=1)
    assert (res16.astype(L)[sel] >= res[sel]).all(), "res16 below |a - a16|: not an upper bound"
    assert (res16.astype(L)[sel] <= (1 + L(1e-6)) * res[sel] + L(1e-14) * np.sqrt(L(d)) * amax[sel]).all(), "res16 vacuous"
    worst_l1 = float(np.max(np.where(bound[sel] > 0, err[sel] / np.where(bound[sel] > 0, bound[sel], 1), 0)))
    nz = sel[res[sel] > 0]
    worst_res = float(np.max(res16[nz].astype(L) / res[nz])) if nz.size else 1.0
    return worst_l1, worst_res


def check_special_rows(A, planes, scale, l1, at):
    """the rows special_rows() put at `at` .. `at` + 3 (reversed when at > 0)"""
    A = np.asarray(A, dtype=np.float64)
    d = A.shape[1]
    zero, ext = (at, at + 1) if at == 0 else (at + 3, at + 2)
    assert not A[zero].any() and scale[zero] == 1.0 and l1[zero] == 0.0 and not planes[:, zero].any()
    q = planes[0, ext].astype(np.int64) * 65536 + planes[1, ext].astype(np.int64) * 256 + planes[2, ext]
    assert scale[ext] == PREP_MAX == np.abs(A[ext]).max()
    for k in np.flatnonzero(np.abs(A[ext]) == PREP_MAX):
        sign = 1 if A[ext, k] > 0 else -1
        assert q[k] == sign * int(fb.F) and planes[0, ext, k] == sign * 127


# ---- 2. the gap table -----------------------------------------------------------------------------------------------
GAP_SHAPES = ((130, 16), (700, 96), (1985, 32))       # proto_gap_kernel<1> with M % 64 and M % 32 != 0, and <2>
GAP_GENERATORS = ("blobs", "tiny_spread_large_mean", "offset_blobs", "tiny_and_huge_rows")
GAP_N = 300
GAP_BAD_ROWS = (5, 7)                                  # bad=True: a NaN row and a row with an infinity
GAP_INPUTS = tuple((name, False) for name in GAP_GENERATORS) + (("blobs", True),)


def gap_inputs(name, M, d, bad=False):
    """the distributions of test_filter_bound.CASES at M prototypes, GAP_N samples and d features, with the
    duplicate W[1] = W[0] and the near duplicate W[2] = W[0] (1 + 1e-13) -> (X float32, W float64)"""
    rng = _rng("gap", name, M, d)
    N = GAP_N
    if name == "blobs":
        X = (rng.normal(size=(4, d)) * 4)[rng.integers(0, 4, N)] + rng.normal(size=(N, d))
        W = rng.normal(size=(M, d)) * 4
    elif name == "tiny_spread_large_mean":
        X, W = rng.uniform(0.45, 0.55, size=(N, d)), rng.uniform(0.45, 0.55, size=(M, d))
    elif name == "offset_blobs":
        X = 100.0 + rng.normal(size=(5, d))[rng.integers(0, 5, N)] + 0.01 * rng.normal(size=(N, d))
        W = 100.0 + rng.normal(size=(M, d))
    elif name == "tiny_and_huge_rows":
        X = np.concatenate([rng.normal(size=(N // 2, d)) * 1e-6, rng.normal(size=(N - N // 2, d)) * 1e6])
        W = np.concatenate([rng.normal(size=(M // 2, d)) * 1e-6, rng.normal(size=(M - M // 2, d)) * 1e6])
    else:
        raise KeyError(name)
    W[1] = W[0]
    W[2] = W[0] * (1 + 1e-13)
    if bad:
        W[GAP_BAD_ROWS[0]] = np.nan
        W[GAP_BAD_ROWS[1], 3] = np.inf
    return X.astype(np.float32), np.ascontiguousarray(W)


def exact_dist2_down(W):
    """|w_p - w_j|^2 in direct form (sum of squared differences) in np.longdouble, rounded DOWN to float64 by one
    part in 2^50"""
    Wl = np.asarray(W, dtype=L)
    M = Wl.shape[0]
    out = np.empty((M, M), dtype=np.float64)
    down = 1 - L(2) ** -50
    for p0 in range(0, M, 64):
        t = Wl[p0:p0 + 64, None, :] - Wl[None, :, :]
        out[p0:p0 + 64] = ((t * t).sum(axis=2) * down).astype(np.float64)
    return out


def gap_reference(W):
    """-> (exact squared distances rounded down, the emulation's (gap, lo, e), mask of the pairs with a non-finite
    row); the non-finite rows count as zero rows in the first two and are masked by the third"""
    finite = np.isfinite(W).all(axis=1)
    Wz = np.where(finite[:, None], W, 0.0)
    badpair = ~(finite[:, None] & finite[None, :])
    return exact_dist2_down(Wz), fb.proto_gap(Wz), badpair


def check_gap_table(gap, W, ref):
    """every check of issue section 2 on a table (float32 or float64 M x M) -> (worst gap / exact, share of clear pairs)"""
    exact, (egap, lo, e), badpair = ref
    M = W.shape[0]
    g = np.asarray(gap, dtype=np.float64)
    assert g.shape == (M, M)
    ok = ~badpair
    assert (g[ok] <= exact[ok]).all(), "a gap above the squared distance"
    assert np.array_equal(np.asarray(gap), np.asarray(gap).T), "the table is not symmetric bit for bit"
    assert not np.diagonal(g).any(), "a diagonal entry is not 0"
    assert g[0, 1] == 0.0 and g[1, 0] == 0.0, "the duplicate pair has a gap"
    assert not g[badpair].any(), "a pair with a non-finite row has a gap"
    clear = ok & (lo > 10.0 * e)
    assert (g[clear] >= 0.5 * egap[clear]).all(), "a clear pair's gap is below half the emulation's"
    pos = ok & (exact > 0)
    return float(np.max(g[pos] / exact[pos])), float(clear.sum()) / max(int(ok.sum()) - int(np.diagonal(ok).sum()), 1)


# ---- 3. dbgsom_bmu_filtered called raw ------------------------------------------------------------------------------
RAW_SHAPES = ((1, 16, 1), (127, 16, 2), (129, 16, 129), (1000, 48, 300), (300, 16, 8200), (131073, 16, 130))   # (N, d, M)
RAW_DTYPES = ("f32", "f64", "f32r")                    # f32r: float32 samples, float32-valued prototypes, round_f32 = 1
RAW_PADS = (0, 16)
RAW_PLANES = (0, 1, 2, 3)
RAW_STRIDES = (0, 1, 8, 64)
RAW_FLAGS = {"none": 0, "seed_full": SEED_FULL, "prune": PRUNE, "prune_retry": PRUNE | PRUNE_RETRY, "probe": PRUNE_PROBE,
             "refine": REFINE, "prune_refine": PRUNE | REFINE}
RAW_SEEDS = ("stateless", "winners", "zeros", "random", "farthest", "dup_hi")
# (shape index, dtype, ldx - d, sweep_planes, seed_stride, flags, seeds): every pair of values of every two columns
# occurs in a row (tests/test_filter_device_cpu.py checks that, and the launcher forms the rows reach)
RAW_CASES = (
    (0, 'f32', 0, 0, 0, 'none', 'stateless'),
    (1, 'f64', 16, 1, 1, 'seed_full', 'winners'),
    (2, 'f32r', 0, 2, 8, 'prune', 'zeros'),
    (3, 'f32', 16, 3, 64, 'prune_retry', 'random'),
    (4, 'f64', 0, 0, 64, 'probe', 'farthest'),
    (5, 'f32r', 16, 1, 0, 'refine', 'dup_hi'),
    (0, 'f32', 16, 2, 1, 'prune_refine', 'farthest'),
    (1, 'f64', 0, 3, 8, 'prune_refine', 'dup_hi'),
    (2, 'f32r', 16, 3, 1, 'probe', 'stateless'),
    (4, 'f32', 16, 1, 8, 'none', 'zeros'),
    (3, 'f64', 0, 2, 0, 'seed_full', 'random'),
    (5, 'f32r', 0, 0, 1, 'prune_retry', 'winners'),
    (0, 'f64', 0, 1, 64, 'prune', 'stateless'),
    (1, 'f32', 0, 2, 64, 'refine', 'winners'),
    (2, 'f32', 16, 0, 64, 'seed_full', 'dup_hi'),
    (4, 'f32r', 16, 3, 0, 'prune', 'farthest'),
    (3, 'f64', 0, 0, 8, 'refine', 'zeros'),
    (0, 'f32r', 16, 1, 8, 'probe', 'random'),
    (3, 'f32r', 0, 2, 1, 'none', 'dup_hi'),
    (2, 'f64', 16, 1, 0, 'prune_retry', 'farthest'),
    (5, 'f32r', 0, 3, 64, 'prune_refine', 'zeros'),
    (1, 'f32', 16, 0, 1, 'prune', 'random'),
    (5, 'f32', 0, 2, 8, 'seed_full', 'stateless'),
    (1, 'f32', 16, 2, 0, 'probe', 'zeros'),
    (0, 'f64', 0, 3, 0, 'none', 'winners'),
    (4, 'f64', 16, 3, 1, 'refine', 'stateless'),
    (3, 'f32r', 0, 1, 8, 'prune_refine', 'winners'),
    (4, 'f32', 16, 2, 8, 'prune_retry', 'dup_hi'),
    (0, 'f32r', 0, 3, 1, 'seed_full', 'zeros'),
    (5, 'f64', 16, 0, 64, 'none', 'random'),
    (2, 'f32', 0, 0, 0, 'prune_refine', 'random'),
    (1, 'f32r', 16, 1, 8, 'none', 'farthest'),
    (1, 'f64', 0, 0, 64, 'prune_retry', 'stateless'),
    (2, 'f32', 16, 1, 0, 'prune', 'winners'),
    (3, 'f64', 0, 2, 1, 'probe', 'farthest'),
    (0, 'f32r', 16, 3, 64, 'refine', 'dup_hi'),
    (4, 'f32', 0, 0, 0, 'seed_full', 'winners'),
    (5, 'f64', 16, 1, 1, 'prune', 'farthest'),
    (2, 'f32r', 0, 2, 8, 'refine', 'random'),
    (3, 'f32', 16, 3, 64, 'prune_refine', 'stateless'),
    (5, 'f64', 0, 0, 0, 'probe', 'dup_hi'),
    (0, 'f32r', 16, 1, 1, 'prune_retry', 'zeros'),
    (4, 'f32', 0, 2, 8, 'prune_refine', 'random'),
    (3, 'f64', 16, 3, 64, 'prune', 'dup_hi'),
    (1, 'f32r', 0, 0, 0, 'seed_full', 'farthest'),
    (2, 'f32', 16, 1, 1, 'none', 'stateless'),
    (4, 'f64', 0, 2, 8, 'probe', 'winners'),
    (5, 'f32r', 16, 3, 64, 'refine', 'farthest'),
    # one row beyond the pairs: a stateless call whose stride is kept (the only shape with 128 prototypes left at 8)
    (4, 'f32', 0, 1, 8, 'none', 'stateless'),
)


def raw_call_args(case):
    """-> (N, d, M, x dtype 'f32' / 'f64', ldx, seed_stride argument with the flags OR-ed in, sweep_planes, round_f32,
    hinted)"""
    si, dtype, pad, planes, stride, flags, seeds = case
    N, d, M = RAW_SHAPES[si]
    return N, d, M, ("f64" if dtype == "f64" else "f32"), d + pad, stride | RAW_FLAGS[flags], planes, int(dtype == "f32r"), \
        seeds != "stateless"


def form_line(flag_arg, planes, N, d, M, hinted):
    """one input line of tests/filter_form_check.cpp for a raw call (k = 1; dbgsom_bmu_filtered strips DBGSOM_REFINE
    and asks for the refinement's 192-entry tile instead)"""
    return f"{flag_arg & ~REFINE:#x} {planes} 1 {192 if flag_arg & REFINE else 0} {N} {d} {M} {int(hinted)}"


FORM_FIELDS = ("seed_full", "prune", "prune_probe", "prune_retry", "k2", "seed_stride", "Msub", "Msubpad", "nkt_full",
               "nkt_used", "sweep_planes", "marking", "gap_nb", "refine", "rows0", "exact")


def resolve_forms(lines, workdir):
    """pipes `lines` through tests/filter_form_check.cpp (host C++ compiler) -> one dict per line"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler (c++ / g++) on PATH"
    exe = os.path.join(str(workdir), "filter_form_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "dbgsom_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "filter_form_check.cpp")], check=True)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    forms = []
    for ln in out.strip().splitlines():
        head, _, rest = ln.partition(" ")
        assert head == "ok", ln
        vals = rest.split()
        assert len(vals) == len(FORM_FIELDS)
        forms.append({k: (v if k in ("marking", "exact") else int(v)) for k, v in zip(FORM_FIELDS, vals)})
    assert len(forms) == len(lines)
    return forms


def raw_data(si, dtype):
    """blobs with prototypes drawn near rows, exact duplicates among prototypes and among samples, one zero row
    -> (X as stored, float32 or float64; W float64 -- float32-valued for 'f32r')"""
    N, d, M = RAW_SHAPES[si]
    rng = _rng("raw", si, dtype)
    k = max(1, min(12, M))
    X = (rng.normal(size=(k, d)) * 4)[rng.integers(0, k, N)] + 0.5 * rng.normal(size=(N, d))
    if N >= 2:
        X[0] = 0.0
    if N >= 8:
        X[5] = X[4]
        X[7] = X[4]
    X = da.stored(X, "f64" if dtype == "f64" else "f32")
    W = X[rng.integers(0, N, M)].astype(np.float64) + 0.05 * rng.normal(size=(M, d))
    for _ in range(M // 8):
        lo = int(rng.integers(0, M - 1))
        W[int(rng.integers(lo + 1, M))] = W[lo]
    if dtype == "f32r":
        W = W.astype(np.float32).astype(np.float64)
    return X, np.ascontiguousarray(W)


def raw_seeds(kind, X, W, winners, key):
    """previous winners of a hinted call (int64) and their stable bucket order (int32); None, None: stateless"""
    if kind == "stateless":
        return None, None
    N, M = X.shape[0], W.shape[0]
    rng = _rng("seeds", key)
    if kind == "winners":
        prev = winners.copy()
    elif kind == "zeros":
        prev = np.zeros(N, dtype=np.int64)
    elif kind == "random":
        prev = rng.integers(0, M, N)
    elif kind == "farthest":
        prev = np.empty(N, dtype=np.int64)
        ww = (W * W).sum(axis=1)
        for s in range(0, N, 16384):
            prev[s:s + 16384] = np.argmax(ww[None, :] - 2.0 * (X[s:s + 16384].astype(np.float64) @ W.T), axis=1)
    elif kind == "dup_hi":                               # the highest-indexed copy of the winner's row
        _, inv = np.unique(W, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        top = np.zeros(inv.max() + 1, dtype=np.int64)
        np.maximum.at(top, inv, np.arange(M))
        prev = top[inv[winners]]
        assert (prev >= winners).all() and (W[prev] == W[winners]).all()
    else:
        raise KeyError(kind)
    prev = np.ascontiguousarray(prev, dtype=np.int64)
    return prev, np.argsort(prev, kind="stable").astype(np.int32)


def check_counts(counts, N, M, order, winners):
    """candidate-list lengths of the 128-sample workgroups: in [1, M]; hinted (order given): at least the number of
    distinct true winners among the workgroup's samples"""
    nb = (N + 127) // 128
    assert counts.shape == (nb,)
    assert (counts >= 1).all() and (counts <= M).all(), (int(counts.min()), int(counts.max()), M)
    if order is not None:
        for g in range(nb):
            assert counts[g] >= np.unique(winners[order[128 * g:128 * g + 128]]).size, g


def check_refine_counts(out4, N, M):
    nb = (N + 127) // 128
    pairs, refined, overflowed = int(out4[0]), int(out4[1]), int(out4[2])
    assert refined <= nb and overflowed <= N and pairs <= N * M, (pairs, refined, overflowed)
    if refined >= 1:
        assert pairs >= refined
