"""CPU: the tables of the large-offset tests (tests/large_offsets.py) hold what they claim -- every part A case lies
inside the one allocation without overlaps, crosses the thresholds its geometry names, respects the caps of DESIGN.md
("Offsets above 32 bits") and falls into the kernel class its id names; the part B sizes cross what they claim -- and
the limits that section found unenforced are refused with DBGSOM_EINVAL and a message before any HIP call."""
import os

import numpy as np
import pytest

from tests import device_abi as da
from tests import large_offsets as lo

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from dbgsom_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.load()


def _disjoint_and_inside(spans):
    spans = sorted(spans)
    assert spans[0][0] >= 0 and spans[-1][1] <= lo.TOTAL
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a0 < a1 <= b0 < b1


# every (geometry, d, bytes of a result row) part A uses
def _part_a_uses():
    uses = [(g, d, 0) for g, d in lo.NORM_CASES + lo.COLSUM_CASES + lo.WCOLSUM_CASES]
    uses += [(g, d, 0) for g, d, _M, _c in lo.BMU_CASES] + [(g, d, 0) for g, d, _c in lo.SEGSUM_CASES]
    uses += [(g, d, 8 * M) for g, d, M in lo.DIST_CASES]
    uses += [(g, 37, 8 * 513) for g in lo.MASKED_GEOMS if g in lo.OUT_GEOMS]           # masked / Manhattan matrices
    uses += [(g, 48, 8 * 513) for g in lo.OUT_GEOMS]                                   # cosine matrices
    uses += [(g, d, 0) for g in lo.GEOM for d in (33, 37, 41, 48, 70)]                 # searches, selections, matrix readers
    uses += [(g, lo.FILTER_D, 0) for g in lo.PLANES_GEOMS]
    return uses


def test_geometries_are_just_above_2_to_28_and_aligned_as_named():
    for geom, (dtype, ld) in lo.GEOM.items():
        rb = lo.row_bytes(geom)
        assert 2 ** 28 < rb <= 2 ** 28 + 64, geom
        kind = geom.split("-")[1]
        assert dtype == geom.split("-")[0]
        assert (rb % 16 == 0) == (kind == "al16") and lo.aligned16(geom) == (kind == "al16")
        assert (rb % 8 == 0 and rb % 16 != 0) == (kind == "al8") or kind != "al8"
        assert kind != "odd" or ld % 2 == 1
        assert (geom in lo.OUT_GEOMS) == (rb % 8 == 0)
        if geom in lo.OUT_GEOMS:
            assert lo.out_ld(geom) * 8 == rb
    assert lo.ld_of("f32-odd") == 2 ** 26 + 3 and lo.ld_of("f64-odd") == 2 ** 25 + 3 and lo.ld_of("bf16-al16") == 2 ** 27 + 8


@pytest.mark.parametrize("geom", list(lo.GEOM))
def test_geometry_crosses_what_it_names(geom):
    want = lo.CROSSES[geom]
    for t in ("B31", "B32", "B33", "E31", "E32"):
        first = lo.first_row_past(geom, t)
        if t in want:
            assert first == want[t] and first < lo.ROWS, (geom, t, first)
        else:
            assert first >= lo.ROWS, (geom, t, first)
    # the issue's geometry: rows 8+ past byte 2^31, 16+ past 2^32, 32+ past 2^33; the narrow types past element 2^31
    # (rows 32+ at the latest), bfloat16 past element 2^32
    assert (want["B31"], want["B32"], want["B33"]) == (8, 16, 32)
    dtype = lo.dtype_of(geom)
    assert ("E31" in want) == (dtype != "f64") and ("E32" in want) == (dtype == "bf16")
    if dtype != "f64":
        assert 32 * lo.ld_of(geom) >= 2 ** 31
    if dtype == "bf16":
        assert 32 * lo.ld_of(geom) >= 2 ** 32


def test_every_case_lies_inside_the_allocation_without_overlap():
    assert lo.TOTAL == 2 ** 33 + 2 ** 30 and lo.ROWS == 35
    for geom, d, out_bytes in _part_a_uses():
        assert out_bytes <= lo.WINDOW
        if out_bytes:
            assert geom in lo.OUT_GEOMS
        assert d * da.ITEM[lo.dtype_of(geom)] <= lo.WINDOW           # a row ends in front of its window
        _disjoint_and_inside(lo.spans(geom, d, out_bytes))
    # the densified rows are zero-filled over N x ld elements
    for geom in lo.DENSIFY_GEOMS:
        assert lo.ROWS * lo.row_bytes(geom) <= lo.TOTAL and (lo.ROWS * lo.row_bytes(geom)) % 8 == 0


def test_cases_respect_the_caps():
    for geom in lo.MASKED_GEOMS:
        assert lo.dtype_of(geom) in ("f32", "f64") and lo.ld_of(geom) <= lo.MASKED_LD_CAP
        assert 16 * lo.ld_of(geom) < 2 ** 32                         # uint32 off[R] of direct_rows.h, R = 16 rows
    for geom in lo.FILTER_GEOMS:
        assert lo.aligned16(geom) and lo.dtype_of(geom) in ("f32", "f64") and lo.FILTER_D % 64 == 0
    assert set(lo.FILTER_GEOMS) <= set(lo.PLANES_GEOMS)
    assert {lo.dtype_of(g) for g in lo.PLANES_GEOMS} == {"f32", "f64", "bf16"}         # every storage type of the planes
    assert "E32" in lo.CROSSES["bf16-al16"] and "bf16-al16" in lo.PLANES_GEOMS          # rows past element 2^32
    assert any(not lo.aligned16(g) for g in lo.PLANES_GEOMS)
    assert lo.ROWS < 2 ** 31 - 1 and lo.TALL_N < 2 ** 31 - 1         # N of the sums, the sort and the context
    assert lo.KN_M <= da.MAX_PROTOTYPES and lo.QUERY_M <= da.MAX_PROTOTYPES
    assert -(-lo.ROWS // lo.KN_SLAB_ROWS) == 3                       # three slabs


@pytest.mark.parametrize("geom,d,M,cls", lo.BMU_CASES, ids=lo.BMU_IDS)
def test_bmu_cases_fall_into_their_class(geom, d, M, cls):
    dtype, ld = lo.GEOM[geom]
    got = da.bmu_class(dtype, d, ld, 0, 0, M)
    assert got[0] == cls
    # a compact stride of the same class exists (what the far result is compared with bit for bit)
    assert any(da.bmu_class(dtype, d, c, 0, 0, M) == got for c in (d, d + 1, d + 2, d + 4, d + 8))


def test_bmu_cases_cover_both_kernels_and_both_map_sizes():
    for dtype in ("f32", "f64"):
        mine = [(c[2], c[3]) for c in lo.BMU_CASES if lo.dtype_of(c[0]) == dtype]
        assert {("dma", 3), ("dma", 257)} <= {(cls, M) for M, cls in mine} and any(cls == "reg" for _M, cls in mine)
    assert {c[2] for c in lo.BMU_CASES if lo.dtype_of(c[0]) == "bf16"} == {3, 257}


@pytest.mark.parametrize("geom,d,cls", lo.SEGSUM_CASES, ids=lo.SEGSUM_IDS)
def test_segsum_cases_fall_into_their_class(geom, d, cls):
    dtype, ld = lo.GEOM[geom]
    assert da.segsum_class(dtype, d, ld, 0) == cls
    assert any(da.segsum_class(dtype, d, c, 0) == cls for c in (d, d + 1, d + 2, d + 4, d + 8))


def test_segsum_cases_cover_every_vector_width_and_both_branches():
    got = {(lo.dtype_of(g), c) for g, _d, c in lo.SEGSUM_CASES}
    for dtype, v in (("f32", 4), ("f64", 2), ("bf16", 8)):
        assert {(dtype, (v, "lanes")), (dtype, (v, "wide")), (dtype, (1, "lanes"))} <= got
    rng = np.random.default_rng(0)
    win = lo.acc_winners(rng)
    assert np.array_equal(np.bincount(win, minlength=lo.ACC_M), lo.ACC_COUNTS) and lo.ACC_COUNTS[1] == 0


def test_compact_strides_keep_the_alignment_class():
    for geom in lo.MASKED_GEOMS:
        for d in (1, 4, 37, 48):
            ldc = lo.same_alignment_ld(geom, d)
            assert d <= ldc <= d + 3 and da.aligned16(ldc, 0, lo.dtype_of(geom)) == lo.aligned16(geom)


def test_random_rows_are_distinct_and_stored_as_named():
    for geom in lo.GEOM:
        A = lo.random_rows(geom, 33, 1)
        assert A.shape == (lo.ROWS, 33) and A.dtype == lo.NP_DTYPE[lo.dtype_of(geom)]


def test_tall_sizes_cross_what_they_claim():
    _dt, N, d = lo.T32
    assert N == 2 ** 21 + 8192 + 17 and N * d > 2 ** 31 and N * d * 4 > 2 ** 33
    assert 3 * N * d > 2 ** 32                                       # the digit planes (d = 1024 is its own padded form)
    _dt, N16, d16 = lo.T16
    assert N16 == N and N16 * d16 > 2 ** 32 and N16 * d16 * 2 > 2 ** 33
    assert N * lo.QUERY_M * 8 > 2 ** 32
    assert lo.TALL_M == 64 < lo.FILTER_MIN_M <= max(s * s for s in lo.TALL_SIDES)
    assert d % 16 == 0 and d16 % 16 == 0                             # the context borrows the rows as they are
    rows = lo.picked_rows("f32", N, d)
    assert len(rows) <= 4 * lo.PICK and rows[-1] == N - 1 and np.array_equal(rows, np.unique(rows))
    for first in (2 ** 31 // d, 2 ** 32 // (4 * d)):                  # the rows on either side of element 2^31 / byte 2^32
        assert first - 1 in rows and first in rows and first + lo.PICK // 2 - 1 in rows
    assert (2 ** 31 // d) * d == 2 ** 31 and (2 ** 32 // (4 * d)) * 4 * d == 2 ** 32     # (rows start on both thresholds)
    rows16 = lo.picked_rows("bf16", N16, d16)
    assert 2 ** 32 // d16 - 1 in rows16 and 2 ** 32 // d16 in rows16 and rows16[-1] == N16 - 1      # element 2^32
    assert lo.PEAK_BYTES >= N * d * 4 + 3 * N * d + N * lo.QUERY_M * 8


# ---- the refusals added with the table -----------------------------------------------------------------------------------
P = 4096    # a pointer that is never followed: the calls below return before any HIP call


def test_filter_calls_refuse_rows_longer_than_an_int(lib):
    def failed(rc, fn, what):
        msg = lib.dbgsom_last_error()
        assert rc == EINVAL and fn in msg and what in msg, (rc, msg)

    d = 2 ** 31 - 64 + 16
    rc = lib.dbgsom_filter_prepare(P, da.F32, 10, d, d, P, 1 << 62, None)
    failed(rc, b"dbgsom_filter_prepare", b"rows longer than 2^31 - 64 values")
    for dtype in (da.F64, da.BF16):
        assert lib.dbgsom_filter_prepare(P, dtype, 10, 2 ** 40, 2 ** 40, P, 1 << 62, None) == EINVAL
    rc = lib.dbgsom_bmu_filtered(P, da.F32, 10, d, d, P, P, P, 5, P, None, None, 0, 0, 0, P, P, P, 1 << 62, None)
    failed(rc, b"launch_bmu_filtered", b"rows longer than 2^31 - 64 values")
    # the caps that were there already still speak
    assert lib.dbgsom_bmu_masked(P, da.F32, 10, 4, 2 ** 27 + 1, P, 3, 4, 1, P, P, P, 1 << 40, None) == EINVAL
    assert b"2^27" in lib.dbgsom_last_error()
    assert lib.dbgsom_accumulate(P, da.F32, 2 ** 31 - 1, 4, 4, P, P, P, 3, P, None, P, 1 << 62, None) == EINVAL
    assert b"bad sample shape" in lib.dbgsom_last_error()
