"""Tables and placement helpers of the large-offset tests (tests/test_gpu_large_offsets.py,
tests/test_large_offsets_cpu.py): rows more than 2^32 bytes from the pointer a raw call of include/dbgsom_hip.h is
given (part A), and compact matrices with more than 2^31 / 2^32 elements behind the context (part B).

Part A.  One allocation of TOTAL bytes, filled with 0xff (every float type reads NaN, every integer -1), holds ROWS
rows `ld` elements apart with the byte stride RB = ld * itemsize just above 2^28: rows 8+ lie past byte 2^31, rows
16+ past 2^32, rows 32+ past 2^33; float32 and bfloat16 rows 32+ past element 2^31, bfloat16 rows 32+ past element
2^32.  Results that take a leading dimension are written into the same allocation at the same byte stride, WINDOW
bytes behind each input row (a window of at most WINDOW bytes): outputs past 2^32 bytes cost no second buffer.

Nothing here needs a GPU: the CPU file checks that every case lies inside the allocation, crosses what its
geometry's name promises, respects the caps of DESIGN.md ("Offsets above 32 bits") and falls into the kernel class
its id names (the launcher branches restated in tests/device_abi.py)."""
import numpy as np

from tests import device_abi as da

TOTAL = 2 ** 33 + 2 ** 30       # bytes of the one allocation (9 GiB)
ROWS = 35
WINDOW = 2 ** 20                # an output row starts this many bytes behind its input row and is at most as long
MASKED_LD_CAP = 2 ** 27         # masked_check_shape (masked.hip): the masked and Manhattan forms
NP_DTYPE = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16}

# geometry -> (dtype, ld in elements).  al16: base and stride multiples of 16 bytes (LDS-DMA and vector classes);
# al8: multiples of 8 and not of 16 (the stride a float64 output can share: ldo = RB / 8); odd: ld odd.
GEOM = {
    "f32-al16": ("f32", 2 ** 26 + 4), "f32-al8": ("f32", 2 ** 26 + 2), "f32-odd": ("f32", 2 ** 26 + 3),
    "f64-al16": ("f64", 2 ** 25 + 2), "f64-odd": ("f64", 2 ** 25 + 3),
    "bf16-al16": ("bf16", 2 ** 27 + 8), "bf16-al8": ("bf16", 2 ** 27 + 4), "bf16-odd": ("bf16", 2 ** 27 + 3),
}
# what each geometry crosses: threshold -> the first row that starts past it.  B31: byte 2^31 from the base, E32:
# element 2^32 from the base.  (float64 rows stay below element 2^31: 34 (2^25 + 3) < 2^31.)
CROSSES = {
    "f32-al16": {"B31": 8, "B32": 16, "B33": 32, "E31": 32},
    "f32-al8": {"B31": 8, "B32": 16, "B33": 32, "E31": 32},
    "f32-odd": {"B31": 8, "B32": 16, "B33": 32, "E31": 32},
    "f64-al16": {"B31": 8, "B32": 16, "B33": 32},
    "f64-odd": {"B31": 8, "B32": 16, "B33": 32},
    "bf16-al16": {"B31": 8, "B32": 16, "B33": 32, "E31": 16, "E32": 32},
    "bf16-al8": {"B31": 8, "B32": 16, "B33": 32, "E31": 16, "E32": 32},
    "bf16-odd": {"B31": 8, "B32": 16, "B33": 32, "E31": 16, "E32": 32},
}


def dtype_of(geom):
    return GEOM[geom][0]


def ld_of(geom):
    return GEOM[geom][1]


def row_bytes(geom):
    """RB: the byte stride of the rows"""
    dtype, ld = GEOM[geom]
    return ld * da.ITEM[dtype]


def row_byte(geom, r):
    return r * row_bytes(geom)


def out_byte(geom, r):
    return r * row_bytes(geom) + WINDOW


def out_ld(geom, item=8):
    """the leading dimension, in elements of `item` bytes, of a result stored at the rows' byte stride"""
    assert row_bytes(geom) % item == 0, f"{geom}: RB is no multiple of {item}"
    return row_bytes(geom) // item


def first_row_past(geom, threshold):
    """the first row whose first byte (B..) or first element (E..) lies at or past 2^n"""
    unit = row_bytes(geom) if threshold[0] == "B" else ld_of(geom)
    return -(-(2 ** int(threshold[1:])) // unit)


def spans(geom, d, out_row_bytes=0, rows=ROWS):
    """the byte intervals a case touches: [start, end) of every input row and of every output window"""
    item = da.ITEM[dtype_of(geom)]
    s = [(row_byte(geom, r), row_byte(geom, r) + d * item) for r in range(rows)]
    if out_row_bytes:
        s += [(out_byte(geom, r), out_byte(geom, r) + out_row_bytes) for r in range(rows)]
    return s


def aligned16(geom):
    return da.aligned16(ld_of(geom), 0, dtype_of(geom))


# ---- part A case tables ----------------------------------------------------------------------------------------------
# dbgsom_row_sqnorms: (geometry, d)
NORM_CASES = [(g, d) for g in GEOM for d in (33, 48)]

# dbgsom_bmu: (geometry, d, M, class): 'dma' the LDS-DMA kernel, 'reg' the register-staged one (device_abi.bmu_class);
# every case at k = 1 and k = 2
BMU_CASES = [
    ("f32-al16", 48, 3, "dma"), ("f32-al16", 48, 257, "dma"), ("f32-al16", 40, 257, "reg"), ("f32-odd", 33, 3, "reg"),
    ("f32-odd", 48, 257, "reg"),
    ("f64-al16", 48, 3, "dma"), ("f64-al16", 48, 257, "dma"), ("f64-al16", 40, 3, "reg"), ("f64-odd", 33, 257, "reg"),
    ("bf16-al16", 48, 3, "reg"), ("bf16-al16", 48, 257, "reg"), ("bf16-odd", 33, 257, "reg"), ("bf16-odd", 48, 3, "reg"),
]
BMU_IDS = ["%s-d%d-M%d-%s" % c for c in BMU_CASES]

# dbgsom_column_sums (float32 / float64) and dbgsom_weighted_column_sums: (geometry, d)
COLSUM_CASES = [("f32-al16", 48), ("f32-odd", 37), ("f64-al16", 48), ("f64-odd", 37)]
WCOLSUM_CASES = COLSUM_CASES + [("bf16-al16", 48), ("bf16-odd", 37)]

# dbgsom_accumulate[_weighted]: (geometry, d, segsum_kernel class as device_abi.segsum_class returns it); crafted
# winners over M = 6 with one empty neuron
SEGSUM_CASES = [
    ("f32-al16", 48, (4, "lanes")), ("f32-al16", 1028, (4, "wide")), ("f32-odd", 37, (1, "lanes")),
    ("f32-odd", 257, (1, "wide")), ("f32-al8", 48, (1, "lanes")),
    ("f64-al16", 34, (2, "lanes")), ("f64-al16", 514, (2, "wide")), ("f64-odd", 37, (1, "lanes")),
    ("bf16-al16", 64, (8, "lanes")), ("bf16-al16", 2056, (8, "wide")), ("bf16-odd", 37, (1, "lanes")),
    ("bf16-al8", 64, (1, "lanes")),
]
SEGSUM_IDS = ["%s-d%d-v%d-%s" % (g, d, c[0], c[1]) for g, d, c in SEGSUM_CASES]
ACC_M = 6
ACC_COUNTS = [12, 0, 1, 9, 8, 5]     # rows per neuron: they add up to ROWS, neuron 1 is empty

# the float32 / float64 geometries of the forms with missing entries and of metric="manhattan" (ldx <= 2^27)
MASKED_GEOMS = ["f32-al16", "f32-odd", "f64-al16", "f64-odd"]
# geometries whose byte stride a float64 result can share (RB a multiple of 8)
OUT_GEOMS = ["f32-al16", "f32-al8", "f64-al16", "f64-odd", "bf16-al16", "bf16-al8"]

# dbgsom_distances* with far ldx and far ldo: (geometry, d, M); M = 513 makes three prototype chunks of 256
DIST_CASES = [(g, d, M) for g in OUT_GEOMS for d, M in ((48, 3), (33, 513))]
DIST_IDS = ["%s-d%d-M%d" % c for c in DIST_CASES]
# dbgsom_kneighbors*: slab_rows = 16 makes three slabs of the 35 rows
KN_SLAB_ROWS = 16
KN_K = 5
KN_M = 40

# dbgsom_csr_densify zero-fills ROWS x ld elements: geometries whose ROWS x RB bytes are whole 8-byte words
DENSIFY_GEOMS = ["f32-al16", "f32-al8", "f64-al16", "f64-odd"]

# the filtered search (d % 64 == 0, float32 / float64, 16-byte aligned rows)
FILTER_GEOMS = ["f32-al16", "f64-al16"]
FILTER_D, FILTER_M = 64, 24
# dbgsom_filter_prepare and dbgsom_anchor_runs_build take every storage type at any stride
PLANES_GEOMS = FILTER_GEOMS + ["f32-odd", "f64-odd", "bf16-al16", "bf16-odd"]


def same_alignment_ld(geom, d):
    """a small stride with the geometry's 16-byte alignment class (what the kernels of dbgsom_accumulate_masked are
    chosen by: 16-byte pieces when base and stride allow them, single elements otherwise)"""
    item = da.ITEM[dtype_of(geom)]
    per = 16 // item
    if aligned16(geom):
        return -(-d // per) * per
    return d if (d * item) % 16 else d + 1


def acc_winners(rng):
    """35 winners with ACC_COUNTS rows per neuron, shuffled"""
    assert sum(ACC_COUNTS) == ROWS and len(ACC_COUNTS) == ACC_M
    return da.winners_with_counts(ACC_COUNTS, rng)


def random_rows(geom, d, seed, scale=1.5):
    """ROWS pairwise distinct random rows as stored for the geometry's dtype (bfloat16: uint16 bit patterns)"""
    rng = np.random.default_rng(seed)
    A = da.stored(rng.normal(size=(ROWS, d)) * scale, dtype_of(geom))
    assert len({r.tobytes() for r in A}) == ROWS
    return A


# ---- part B ------------------------------------------------------------------------------------------------------------
TALL_N = 2 ** 21 + 8192 + 17
T32 = ("f32", TALL_N, 1024)      # 2.16e9 elements (> 2^31), 8.6e9 bytes (> 2^33); its three digit planes 6.5e9 bytes
T16 = ("bf16", TALL_N, 2048)     # 4.3e9 elements (> 2^32)
TALL_M = 64
FILTER_MIN_M = 129               # SearchPolicy::FILTER_MIN_PROTOTYPES: smaller maps take the all-pairs search
TALL_SIDES = (8, 12)             # lattices of the tall epochs: M = 64, and M = 144 where the filtered search engages
QUERY_M = 300                    # TALL_N x 300 float64 distances: 5.05e9 bytes (> 2^32)
PEAK_BYTES = 25 * 10 ** 9        # samples + planes + workspaces + the distance matrix, whichever test holds most
PICK = 512


def picked_rows(dtype, N, d, seed=0):
    """the rows the tall tests compare with the oracle: the last PICK, PICK around element 2^31, around element 2^32
    (where the matrix has one) and around byte 2^32 of the compact matrix, and PICK at random -- sorted, without
    duplicates"""
    item = da.ITEM[dtype]
    rng = np.random.default_rng(seed)
    centres = [c for c in (2 ** 31 // d, 2 ** 32 // (d * item), 2 ** 32 // d) if c < N]
    rows = [np.arange(N - PICK, N), rng.choice(N, PICK, replace=False)]
    for c in centres:
        lo = max(0, min(N - PICK, c - PICK // 2))
        rows.append(np.arange(lo, lo + PICK))
    return np.unique(np.concatenate(rows)).astype(np.int64)
