"""Helpers of the device-level ABI tests (tests/test_gpu_device_abi.py, tests/test_device_abi_cpu.py): raw calls
of include/dbgsom_hip.h with unpadded, strided and unaligned rows -- what the context never passes.

Staging: rows of `ld` elements whose columns d .. ld hold NaN (a read of padding poisons the result), row 0
`offset_elems` elements into the allocation.  bfloat16 rows travel as their bit patterns (uint16); the references
see the exactly widened values.  References are NumPy only: the order-pinned chains of oracle/ bit for bit, and for
the sums np.longdouble (64-bit significand) sums of the terms with T = sum |term| beside them.

The shape tables live here so that the CPU file can check, without a GPU, that every table holds the launcher
branches it claims (the formulas of accumulate.hip, bmu.hip, bmu_dma.hip and smooth.hip restated below)."""
import ctypes
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53           # unit roundoff of float64
UL = 2.0 ** -64          # unit roundoff of np.longdouble (x87 extended: 64-bit significand)
F32, F64, BF16 = 0, 1, 2
CODE = {"f32": F32, "f64": F64, "bf16": BF16}
ITEM = {"f32": 4, "f64": 8, "bf16": 2}
MAX_PROTOTYPES = 16000
AT, CH = 256, 128        # accumulate.hip: threads per workgroup, rows per chunk


# ---- storage ------------------------------------------------------------------------------------------------------
def bf16_bits(A32):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even"""
    b = np.ascontiguousarray(A32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def widen(A):
    """the values the device computes with: uint16 bfloat16 bits widen exactly to float32"""
    if A.dtype == np.uint16:
        return (A.astype(np.uint32) << 16).view(np.float32)
    return A


def stored(A, dtype):
    """values -> what is stored for `dtype` ('f32' / 'f64' / 'bf16': uint16 bit patterns)"""
    if dtype == "bf16":
        return bf16_bits(np.asarray(A, dtype=np.float32))
    return np.ascontiguousarray(A, dtype=np.float32 if dtype == "f32" else np.float64)


def host_rows(A, ld, offset_elems):
    """the host image of stage(): NaN everywhere (in front of row 0 and in the columns d .. ld), the rows of A at
    offset_elems + r * ld"""
    rows, d = A.shape
    assert ld >= d and offset_elems >= 0
    if A.dtype == np.uint16:
        buf = np.full(offset_elems + rows * ld, 0x7fc0, dtype=np.uint16)       # the bfloat16 quiet NaN
    else:
        buf = np.full(offset_elems + rows * ld, np.nan, dtype=A.dtype)
    body = buf[offset_elems:].reshape(rows, ld)
    body[:, :d] = A
    return buf


def stage(A, ld, offset_elems, dtype):
    """-> (device tensor, pointer of row 0).  A: as stored() returns it."""
    import torch

    assert A.dtype == {"f32": np.float32, "f64": np.float64, "bf16": np.uint16}[dtype]
    buf = host_rows(A, ld, offset_elems)
    t = torch.from_numpy(buf.view(np.int16) if dtype == "bf16" else buf).cuda()
    assert t.data_ptr() % 256 == 0          # the allocator's alignment: only offset_elems moves row 0 off 16 bytes
    return t, t.data_ptr() + offset_elems * ITEM[dtype]


def workspace(nbytes):
    """-> (tensor, 256-byte aligned pointer) of `nbytes` zero bytes"""
    import torch

    t = torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device="cuda")
    return t, (t.data_ptr() + 255) // 256 * 256


GUARD_FRONT, GUARD_BACK = 256, 4096      # least guard bytes in front of and behind a guarded workspace's body
GUARD_BYTE = 0xA5                         # what the guards hold: neither of the body fills below
BODY_FILL = {"zero": 0x00, "ff": 0xFF}    # "ff": every float reads NaN, every integer -1 or UINT_MAX


def guards_intact(image, body_off, nbytes, guard=GUARD_BYTE):
    """-> (front intact, back intact) of the host image (uint8) of a guarded allocation whose body is
    image[body_off : body_off + nbytes]: every byte outside the body still holds `guard`"""
    image = np.asarray(image, dtype=np.uint8)
    assert 0 <= body_off and body_off + nbytes <= image.size
    return bool((image[:body_off] == guard).all()), bool((image[body_off + nbytes:] == guard).all())


class GuardedWorkspace:
    """[front guard >= GUARD_FRONT bytes | body of exactly `nbytes` bytes, 256-byte aligned | back guard >=
    GUARD_BACK bytes] on the device.  The guards hold GUARD_BYTE, the body whatever `fill` / `reguard` left there; an
    entry is called with (ptr, a size <= nbytes) and `guards_intact` then tells, on the host, whether it wrote in
    front of or behind what it was given.

    What this cannot see: a stray READ past the end (the guards are ordinary, readable memory, and a kernel that reads
    them and throws the value away leaves no trace), a write past the back guard's 4096 bytes, and a write of a byte
    that happens to equal GUARD_BYTE."""

    def __init__(self, nbytes):
        import torch

        self.nbytes = int(nbytes)
        self.t = torch.full((GUARD_FRONT + 256 + self.nbytes + GUARD_BACK,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.off = GUARD_FRONT + (-(self.t.data_ptr() + GUARD_FRONT)) % 256
        self.ptr = self.t.data_ptr() + self.off
        assert self.ptr % 256 == 0 and self.off >= GUARD_FRONT

    def fill(self, kind):
        """the whole body to one of BODY_FILL"""
        self.t[self.off:self.off + self.nbytes] = BODY_FILL[kind]

    def reguard(self, used):
        """an entry is about to be given the first `used` bytes only: what lies behind them becomes guard (the first
        `used` bytes keep what they hold)"""
        assert 0 <= used <= self.nbytes
        self.t[self.off + used:] = GUARD_BYTE

    def intact(self, used=None):
        """-> (front intact, back intact) around the first `used` bytes (default: the whole body)"""
        import torch

        torch.cuda.synchronize()
        return guards_intact(self.t.cpu().numpy(), self.off, self.nbytes if used is None else used)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- launcher branches, restated ----------------------------------------------------------------------------------
def aligned16(ld, offset_elems, dtype):
    """rows whose base and pitch are multiples of 16 bytes (the allocation itself is)"""
    return (offset_elems * ITEM[dtype]) % 16 == 0 and (ld * ITEM[dtype]) % 16 == 0


def finalize_groups(M):
    g = 512 // max(M, 1)
    return 1 if g < 1 else (32 if g > 32 else g)


def hs_for(N):
    return 512 if N <= 300000 else 2048


def segsum_class(dtype, d, ld, offset_elems):
    """-> (VEC, 'wide' | 'lanes'): the segsum_kernel instantiation and its branch (Q = d / VEC >= 256 or row lanes)"""
    v = {"f32": 4, "f64": 2, "bf16": 8}[dtype]
    if not (aligned16(ld, offset_elems, dtype) and d % v == 0):
        v = 1
    return v, ("wide" if d // v >= AT else "lanes")


def dma_chunk_tiles(dtype, M):
    n1, n2, n4 = (M + 31) // 32, (M + 63) // 64, (M + 127) // 128
    if dtype == "f32":
        c1, c2, c4 = 1.00 * n1, 1.74 * n2, 3.33 * n4
        return 4 if (c4 <= c2 and c4 <= c1) else (2 if c2 <= c1 else 1)
    c1, c2, cg = 1.00 * n1, 1.66 * n2, 3.6 * n4
    if cg <= c1 and cg <= c2:
        return 0
    return 2 if c2 <= c1 else 1


def bmu_class(dtype, d, ldx, x_off, w_off_bytes, M):
    """-> ('dma', tiles) or ('reg', xvec, wvec): the kernel launch_bmu picks"""
    xal, wal = aligned16(ldx, x_off, dtype), w_off_bytes % 16 == 0
    if dtype != "bf16" and d % 16 == 0 and xal and wal and dma_chunk_tiles(dtype, M) != 0:
        return ("dma", dma_chunk_tiles(dtype, M))
    return ("reg", int(xal), int(wal and d % 2 == 0))


def gemm_splits(M, d):
    tiles, nkt = ((d + 63) // 64) * ((M + 63) // 64), (M + 15) // 16
    ks = min((768 + tiles - 1) // tiles, 8, nkt // 4)
    return max(ks, 1)


# ---- shape tables ---------------------------------------------------------------------------------------------------
# dbgsom_row_sqnorms: (rows, d, ld); each with and without a one-element base offset, three storage types
NORM_SHAPES = [(1, 1, 1), (9, 15, 15), (8, 16, 19), (17, 1025, 1031), (16385, 33, 35)]

# dbgsom_bmu, register-staged kernel: (dtype, N, d, M, pad, x_off, w_off elements, k, round_f32); ldx = d + pad
BMU_CASES = [
    ("f32", 1, 1, 1, 0, 0, 0, 1, 0), ("f32", 127, 3, 2, 3, 0, 0, 2, 0), ("f32", 129, 15, 129, 0, 1, 0, 1, 1),
    ("f32", 127, 17, 257, 3, 0, 0, 2, 0), ("f32", 129, 33, 129, 3, 0, 0, 1, 1), ("f32", 129, 33, 257, 0, 0, 0, 2, 0),
    ("f32", 1, 17, 2, 0, 1, 0, 2, 1), ("f32", 129, 18, 129, 2, 0, 0, 2, 0), ("f32", 127, 18, 2, 0, 1, 0, 1, 0),
    ("f32", 129, 18, 257, 2, 0, 1, 1, 0),
    ("f64", 1, 3, 1, 0, 0, 0, 1, 0), ("f64", 127, 1, 2, 3, 0, 0, 2, 0), ("f64", 129, 15, 257, 3, 0, 0, 1, 0),
    ("f64", 129, 17, 129, 0, 1, 0, 2, 0), ("f64", 127, 33, 129, 0, 0, 0, 1, 0), ("f64", 129, 33, 257, 3, 0, 0, 2, 0),
    ("f64", 129, 18, 129, 0, 1, 0, 2, 0), ("f64", 127, 18, 257, 0, 0, 0, 1, 0), ("f64", 129, 32, 2, 0, 0, 1, 2, 0),
    ("bf16", 1, 1, 1, 0, 0, 0, 1, 0), ("bf16", 127, 3, 2, 0, 1, 0, 2, 0), ("bf16", 129, 15, 129, 3, 0, 0, 1, 0),
    ("bf16", 129, 17, 257, 7, 0, 0, 2, 0), ("bf16", 127, 33, 129, 7, 0, 0, 1, 0), ("bf16", 129, 33, 257, 0, 0, 0, 2, 0),
    ("bf16", 129, 32, 129, 0, 0, 0, 1, 0), ("bf16", 127, 24, 2, 0, 1, 0, 2, 0), ("bf16", 129, 17, 129, 3, 0, 0, 1, 0),
]
# dbgsom_bmu, LDS-DMA kernel with strided rows: (dtype, N, d, M, ldx)
BMU_DMA_CASES = [("f32", 300, 32, 40, 36), ("f64", 300, 32, 40, 34), ("f32", 300, 32, 32, 36), ("f32", 300, 32, 128, 36)]

# dbgsom_accumulate[_weighted]: every segsum_kernel instantiation.  (dtype, d, pad, offset, weighted); ldx = d + pad.
# d = 2056 also takes the column loop of finalize_kernel (d + 2 > 8 * 256 columns per neuron).
SEGSUM_CASES = [
    ("f32", 1, 0, 0, False), ("f32", 3, 0, 0, False), ("f32", 37, 0, 0, False), ("f32", 37, 0, 0, True),
    ("f32", 255, 0, 0, False), ("f32", 257, 0, 0, False), ("f32", 257, 0, 0, True), ("f32", 48, 4, 0, False),
    ("f32", 48, 4, 0, True), ("f32", 1028, 0, 0, False), ("f32", 1028, 0, 0, True), ("f32", 48, 0, 1, False),
    ("f64", 37, 0, 0, False), ("f64", 37, 0, 0, True), ("f64", 257, 0, 0, False), ("f64", 34, 2, 0, False),
    ("f64", 34, 2, 0, True), ("f64", 514, 0, 0, False),
    ("bf16", 37, 0, 0, False), ("bf16", 37, 0, 0, True), ("bf16", 260, 1, 0, False), ("bf16", 64, 8, 0, False),
    ("bf16", 64, 8, 0, True), ("bf16", 2056, 0, 0, False),
]
SEGSUM_COUNTS = [130, 0, 1, 257, 128, 184]          # rows per neuron of the SEGSUM_CASES (N = 700, M = 6)

# list lengths around the chunk size, M = 40: the named counts, the rest random
LIST_COUNTS_HEAD = [0, 1, 127, 128, 129, 255, 256, 257, 128 * 33 + 1]
# second-level sum of finalize_kernel, d = 8: M -> groups
GROUP_CASES = {1: 32, 16: 32, 17: 30, 256: 2, 257: 1, 513: 1}
GROUP_LONG = 128 * 7 + 5                           # the long list of each GROUP_CASES case: 8 chunks
# scatter kernel: N on both sides of hs_for's switch, and the smallest grids
SCATTER_N = [300001, 300000, 513, 1]

# dbgsom_smooth at odd d: (M, d) -> split-K pieces
SMOOTH_CASES = {(1, 1): 1, (17, 3): 1, (77, 101): 1, (130, 65): 2, (1025, 33): 8, (260, 63): 4}

SUM_N = [0, 1, 255, 257, 70001]
COLSUM_SHAPES = [(1, 1, 1), (1025, 3, 5), (513, 37, 40), (2049, 65, 65)]


def list_counts(rng, M=40):
    counts = np.array(LIST_COUNTS_HEAD + list(rng.integers(0, 60, M - len(LIST_COUNTS_HEAD))), dtype=np.int64)
    return counts[rng.permutation(M)]


def group_counts(rng, M):
    """one long list (GROUP_LONG rows, 8 chunks: it spans the groups whenever there are 2 .. 8 of them per neuron; with
    32 groups every chunk is a group of its own) and short random ones; M = 1: every row in the one neuron"""
    counts = rng.integers(0, 4, M).astype(np.int64)
    counts[M // 2] = GROUP_LONG if M > 1 else 2000
    return counts


def winners_with_counts(counts, rng):
    """a winner vector in which neuron j gets exactly counts[j] rows, shuffled"""
    counts = np.asarray(counts, dtype=np.int64)
    win = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    return win[rng.permutation(win.size)]


# ---- references -----------------------------------------------------------------------------------------------------
def have_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


def segment_sums(terms, winners, M):
    """per-neuron np.longdouble sums of `terms` (N or N x c, float64 or longdouble) in list order and the sums T
    of their magnitudes.  A dot product of n terms evaluated in a format of unit roundoff UL is within about
    n UL T of the exact one: the reference's own error, added to every bound it is used in."""
    terms = np.asarray(terms, dtype=np.longdouble)
    order = np.argsort(winners, kind="stable")
    sw = winners[order]
    shape = (M,) + terms.shape[1:]
    S, T = np.zeros(shape, dtype=np.longdouble), np.zeros(shape, dtype=np.longdouble)
    if sw.size:
        ids, starts = np.unique(sw, return_index=True)
        S[ids] = np.add.reduceat(terms[order], starts, axis=0)
        T[ids] = np.add.reduceat(np.abs(terms[order]), starts, axis=0)
    return S, T


def accumulate_reference(Xw, winners, kw, dist, M, sw=None):
    """(S, K, a, E) and (TS, TK, TE) in np.longdouble for the rows whose winner is inside [0, M); sw: row weights"""
    ok = (winners >= 0) & (winners < M)
    win, X = winners[ok], np.asarray(Xw[ok], dtype=np.longdouble)
    f = np.asarray(kw[ok], dtype=np.longdouble)
    e = np.asarray(dist[ok], dtype=np.longdouble)
    if sw is not None:
        w = np.asarray(sw[ok], dtype=np.longdouble)
        f, e = w * f, w * e
        a = np.asarray(segment_sums(w, win, M)[0], dtype=np.float64)
    else:
        a = np.bincount(win, minlength=M).astype(np.float64)
    S, TS = segment_sums(f[:, None] * X, win, M)
    K, TK = segment_sums(f, win, M)
    E, TE = segment_sums(e, win, M)
    return (S, K, a, E), (TS, TK, TE)


def sums_within_bound(got, ref, T, n, weighted):
    """|got - ref| <= (n + 2) u T (weighted: 2 n + 4: one more rounding per row, the factor sw kw) plus the
    reference's own n UL T (weighted: 2 n UL T).  -> (holds everywhere, largest ratio error / bound)"""
    n = np.asarray(n, dtype=np.longdouble).reshape((-1,) + (1,) * (np.ndim(got) - 1))
    lead = (2 * n + 4) if weighted else (n + 2)
    bound = lead * U * T + (2 if weighted else 1) * n * UL * T
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref)
    ok = bool(np.all(err <= bound))
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0)))) \
        if err.size else 0.0
    return ok, ratio


def accumulate_inputs(dtype, N, d, rng, weights=None):
    """X random (as stored), kw uniform in (0, 1], dist uniform in [0, 3]; weights: None, 'int' (0 .. 3, a fifth of
    the rows at 0) or 'frac'"""
    X = stored(rng.normal(size=(N, d)) * 1.5, dtype)
    kw = 1.0 - rng.random(N)
    dist = 3.0 * rng.random(N)
    sw = None
    if weights is not None:
        sw = rng.integers(0, 4, N).astype(np.float64)
        sw[rng.random(N) < 0.2] = 0.0
        if weights == "frac":
            sw = sw * rng.uniform(0.1, 2.5, N)
    return X, kw, dist, sw


# the inputs of the accumulate tests: (dtype, X as stored, ldx, offset, winners, kw, dist, M, sw, integer weights)
def segsum_case(dtype, d, pad, off, weighted):
    rng = np.random.default_rng(d + pad + off)
    winners = winners_with_counts(SEGSUM_COUNTS, rng)
    X, kw, dist, sw = accumulate_inputs(dtype, winners.size, d, rng, "int" if weighted else None)
    return dtype, X, d + pad, off, winners, kw, dist, len(SEGSUM_COUNTS), sw, True


def list_case(weights):
    rng = np.random.default_rng(40)
    winners = winners_with_counts(list_counts(rng), rng)
    X, kw, dist, sw = accumulate_inputs("f32", winners.size, 20, rng, weights)
    return "f32", X, 20, 0, winners, kw, dist, 40, sw, weights != "frac"


def group_case(M, weighted):
    rng = np.random.default_rng(M)
    winners = winners_with_counts(group_counts(rng, M), rng)
    X, kw, dist, sw = accumulate_inputs("f64", winners.size, 8, rng, "int" if weighted else None)
    return "f64", X, 8, 0, winners, kw, dist, M, sw, True


def histogram_case():
    """M = DBGSOM_MAX_PROTOTYPES: most neurons empty, the last one not"""
    M, N = MAX_PROTOTYPES, 20000
    rng = np.random.default_rng(16)
    winners = rng.choice(rng.choice(M - 1, 3000, replace=False), N).astype(np.int64)
    winners[rng.choice(N, 5, replace=False)] = M - 1
    X, kw, dist, _ = accumulate_inputs("f32", N, 4, rng)
    return "f32", X, 4, 0, winners, kw, dist, M, None, True


def scatter_case(N):
    rng = np.random.default_rng(N)
    winners = rng.integers(0, 5, N).astype(np.int64)
    X, kw, dist, _ = accumulate_inputs("f32", N, 2, rng)
    return "f32", X, 2, 0, winners, kw, dist, 5, None, True


def status_case(weighted, bad):
    """bad: one winner at -1 and one at M"""
    rng = np.random.default_rng(5)
    N, d, M = 1500, 6, 9
    winners = rng.integers(0, M, N).astype(np.int64)
    X, kw, dist, sw = accumulate_inputs("f64", N, d, rng, "int" if weighted else None)
    if bad:
        winners[100], winners[900] = -1, M
    return "f64", X, d, 0, winners, kw, dist, M, sw, True


def smooth_inputs(M, d, rng, nan_row=False):
    """a hand-made [S | K | a | E] buffer with dead neurons (a = K = 0, S = 0), float32 hops on a line cut into two
    disconnected parts (+inf), prototypes to compare with; nan_row: a dead neuron nobody reaches (every h a = 0)"""
    a = rng.integers(1, 50, M).astype(np.float64)
    a[::7] = 0.0 if M > 1 else a[0]
    K = rng.uniform(0.5, 2.0, M) * a
    S = rng.normal(size=(M, d)) * K[:, None]
    S[a == 0] = 0.0
    E = rng.random(M) * a
    hop = np.abs(np.subtract.outer(np.arange(M), np.arange(M))).astype(np.float32)
    cut = M // 3
    if cut:
        part = np.arange(M) < cut
        hop[part[:, None] != part[None, :]] = np.inf
    if nan_row:
        i = 7 if M > 7 else 0
        assert a[i] == 0.0
        hop[i, :] = np.inf
        hop[:, i] = np.inf
        hop[i, i] = 0.0
    W_old = rng.normal(size=(M, d))
    return S, K, a, E, hop, W_old


def exact_sum(v, w=None):
    """-> (sum of v_i, or of v_i w_i, as an exact Fraction; the sum of the terms' magnitudes likewise): integer
    significands shifted onto one exponent"""
    E = -2300
    tot = mag = 0
    for i in range(len(v)):
        m, e = math.frexp(float(v[i]))
        t, e = int(m * 2.0 ** 53), e - 53
        if w is not None:
            m2, e2 = math.frexp(float(w[i]))
            t, e = t * int(m2 * 2.0 ** 53), e + e2 - 53
        t <<= e - E
        tot += t
        mag += abs(t)
    scale = Fraction(1, 2 ** -E)
    return tot * scale, mag * scale


def column_sums_loop(X, mean=None):
    """row by row in X's own dtype, one rounded operation after the other (no fused multiply-add)"""
    acc = np.zeros(X.shape[1], dtype=X.dtype)
    for row in X:
        y = row
        if mean is not None:
            y = row - mean
            y = y * y
        acc = acc + y
    return acc
