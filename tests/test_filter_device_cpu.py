"""CPU companion of tests/test_gpu_filter_device.py: the case tables of tests/filter_device.py hold what they claim
(every pair of option values, every launcher form, the restated layout of the planes buffer), the emulation alone stays
inside every bound the GPU file applies to the gap table, and the argument errors of the raw entry points of the
filtered search come back as status codes before any HIP call."""
import itertools
import os

import numpy as np
import pytest

from tests import device_abi as da
from tests import filter_device as fd
from tests import test_filter_bound as fb


@pytest.fixture(scope="module")
def lib():
    from dbgsom_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.load()


# ---- the tables -------------------------------------------------------------------------------------------------------
def test_raw_cases_are_pairwise():
    dims = [range(len(fd.RAW_SHAPES)), fd.RAW_DTYPES, fd.RAW_PADS, fd.RAW_PLANES, fd.RAW_STRIDES, list(fd.RAW_FLAGS),
            fd.RAW_SEEDS]
    assert all(len(c) == len(dims) and all(v in dim for v, dim in zip(c, dims)) for c in fd.RAW_CASES)
    assert len(set(fd.RAW_CASES)) == len(fd.RAW_CASES) <= 60
    for a, b in itertools.combinations(range(len(dims)), 2):
        seen = {(c[a], c[b]) for c in fd.RAW_CASES}
        assert seen == set(itertools.product(dims[a], dims[b])), (a, b)
    assert fd.RAW_SHAPES == ((1, 16, 1), (127, 16, 2), (129, 16, 129), (1000, 48, 300), (300, 16, 8200), (131073, 16, 130))
    assert fd.GAP_SHAPES == ((130, 16), (700, 96), (1985, 32))


def test_tables_reach_every_launcher_form(tmp_path):
    raw = [fd.raw_call_args(c) for c in fd.RAW_CASES]
    lines = [fd.form_line(flag_arg, planes, N, d, M, hinted) for N, d, M, _, _, flag_arg, planes, _, hinted in raw]
    gaps = [(flag, M, d) for (M, d) in fd.GAP_SHAPES for flag in (fd.PRUNE, fd.PRUNE_PROBE)]
    lines += [fd.form_line(flag, 0, fd.GAP_N, d, M, False) for flag, M, d in gaps]
    forms = fd.resolve_forms(lines, tmp_path)
    for name, case, f in zip(range(len(raw)), fd.RAW_CASES, forms):
        print(f"row {name:2d} {case}: marking {f['marking']}, gap_nb {f['gap_nb']}, exact {f['exact']}, "
              f"seed_stride {f['seed_stride']}, seed_full {f['seed_full']}, prune_retry {f['prune_retry']}")
    rawf, gapf = forms[:len(raw)], forms[len(raw):]
    assert {f["marking"] for f in rawf} == {"prune", "sweep4", "sweep_1_4", "sweep_2_2", "sweep_3_1"}
    assert {f["exact"] for f in rawf} == {"split", "all", "beside_refine"}
    assert any(f["prune_retry"] for f in rawf) and any(f["seed_full"] for f in rawf)
    assert {f["gap_nb"] for f in rawf + gapf} == {0, 1, 2}
    # the gap shapes: <1> twice, then <2>; the pruning form and its counting-only launch beside the default sweep
    assert [f["gap_nb"] for f in gapf] == [1, 1, 1, 1, 2, 2]
    assert [f["marking"] for f in gapf] == ["prune", "sweep_2_2"] * 3
    assert {M % 64 != 0 and M % 32 != 0 for M, _ in fd.GAP_SHAPES} == {True}
    # a caller's stride that is halved (fewer than 128 prototypes would be left) and one that is kept
    stateless = [(a, f) for a, f in zip(raw, rawf) if not a[8] and not f["seed_full"] and (a[5] & 0xff)]
    assert any(f["seed_stride"] < (a[5] & 0xff) for a, f in stateless)
    assert any(f["seed_stride"] == (a[5] & 0xff) > 1 for a, f in stateless)
    # beyond the one-product sweep's bitmask and the gap table: DBGSOM_PRUNE is ignored there
    assert all(f["prune"] == 0 and f["gap_nb"] == 0 for a, f in zip(raw, rawf) if a[2] > fd.PRUNE_MAX_M)
    assert any(f["marking"] == "sweep_1_4" and a[2] == 8200 for a, f in zip(raw, rawf))
    assert any(f["exact"] == "all" and a[0] == 131073 for a, f in zip(raw, rawf))


def test_planes_layout_is_the_librarys(lib):
    shapes = [(r, d) for r in fd.PREP_ROWS for d in fd.PREP_D] + [(N, d) for N, d, _ in fd.RAW_SHAPES] + [(fd.GAP_N, d) for _, d in fd.GAP_SHAPES]
    for rows, d in shapes:
        lay = fd.planes_layout(rows, d)
        assert lay["total"] == lib.dbgsom_filter_planes_bytes(rows, d), (rows, d)
        assert all(lay[k] % 256 == 0 for k in ("planes", "scale", "l1", "res16")) and lay["dpad"] % 64 == 0 and lay["dpad"] >= max(d, 128)
    assert {fd.filter_dpad(d) for d in fd.PREP_D} == {128, 192, 256}
    assert {d % 64 == 0 for d in fd.PREP_D} == {True, False}
    assert lib.dbgsom_filter_planes_bytes(0, 16) == 0 and lib.dbgsom_filter_planes_bytes(5, 0) == 0


def test_prepare_rows_hold_the_special_rows_and_the_emulation_passes_its_own_checks():
    for dtype in fd.PREP_DTYPES:
        for rows in fd.PREP_ROWS:
            for d in fd.PREP_D:
                A = np.asarray(da.widen(fd.prepare_rows(rows, d, dtype)), dtype=np.float64)
                assert A.shape == (rows, d) and np.isfinite(A).all()
                (d0, d1, d2), s, _ = fb.slice_rows(A)
                dpad = fd.filter_dpad(d)
                planes = np.zeros((3, rows, dpad), dtype=np.int8)
                planes[:, :, :d] = np.stack([d0, d1, d2])
                res = fd.residual16(A)
                l1 = np.abs(A).sum(axis=1)
                fd.check_prepared(A, planes, s, l1, (res * (1 + np.longdouble(1e-9))).astype(np.float64) + 1e-300 * (res > 0))
                if rows >= 5:
                    fd.check_special_rows(A, planes, s, l1, 0)
                    huge = A[2]
                    assert np.abs(huge).max() >= 1e5 and np.median(np.abs(huge)) < 1e-4 or d == 1
                    assert np.array_equal(A[3], np.rint(A[3])) and np.abs(A[3]).max() == 4
                if rows >= 131:
                    fd.check_special_rows(A, planes, s, l1, rows - 4)


# ---- the emulation alone is inside the bounds of the gap table's checks ---------------------------------------------
@pytest.mark.parametrize("M,d", fd.GAP_SHAPES)
def test_emulated_gap_stays_under_the_exact_distance(M, d):
    for name, bad in fd.GAP_INPUTS:
        X, W = fd.gap_inputs(name, M, d, bad)
        assert X.shape == (fd.GAP_N, d) and X.dtype == np.float32 and W.shape == (M, d)
        assert np.array_equal(W[1], W[0]) and not np.array_equal(W[2], W[0]) and np.allclose(W[2], W[0], rtol=1e-12, atol=0)
        ref = fd.gap_reference(W)
        # (the kernel reports "no gap known" for a pair with a non-finite row; the emulation never sees such rows)
        worst, clear = fd.check_gap_table(np.where(ref[2], 0.0, ref[1][0]), W, ref)
        print(f"M={M} d={d} {name}{' +nan/inf rows' if bad else ''}: worst emulated gap / exact {worst:.4f}, clear pairs {clear:.5f}")
        assert worst <= 1.0
        if name == "blobs" and not bad:
            assert clear >= 0.99
        if bad:
            assert ref[2].sum() == 2 * (2 * M - 2)          # two non-finite rows: their rows and columns


# ---- argument errors that return before any HIP call ------------------------------------------------------------------
P = 0x10000          # a fake, 256-byte aligned device address: never dereferenced on these paths


def _filtered(lib, *, dtype=da.F32, N=300, d=16, ldx=16, M=130, prev=None, order=None, stride=0, planes=0, ws=P, xplanes=P,
              ws_bytes=None):
    need = lib.dbgsom_bmu_filtered_workspace_bytes(N, d, min(M, fd.FILTER_MAX_M))
    return lib.dbgsom_bmu_filtered(P, dtype, N, d, ldx, P, xplanes, P, M, P, prev, order, stride, planes, 0, P, P, ws,
                                   need if ws_bytes is None else ws_bytes, None)


def test_argument_errors_of_the_filtered_entry_points(lib):
    def failed(rc, code, what=b""):
        msg = lib.dbgsom_last_error()
        assert rc == code and what in msg, (rc, msg)

    EINVAL, ENOMEM = -1, -3
    failed(_filtered(lib, d=24, ldx=24), EINVAL, b"multiple of 16")
    failed(_filtered(lib, prev=P), EINVAL, b"come as a pair")
    failed(_filtered(lib, order=P), EINVAL, b"come as a pair")
    failed(_filtered(lib, stride=65), EINVAL, b"seed_stride")
    failed(_filtered(lib, planes=4), EINVAL, b"sweep_planes")
    failed(_filtered(lib, dtype=da.BF16), EINVAL, b"float32 or float64")
    failed(_filtered(lib, M=16001), EINVAL, b"16000")
    failed(_filtered(lib, ws=P + 64), EINVAL, b"alignment")
    failed(_filtered(lib, xplanes=P + 64), EINVAL, b"alignment")
    need = lib.dbgsom_bmu_filtered_workspace_bytes(300, 16, 130)
    assert need > 256
    failed(_filtered(lib, ws_bytes=need - 1), ENOMEM, b"workspace too small")
    pb = lib.dbgsom_filter_planes_bytes(300, 16)
    failed(lib.dbgsom_filter_prepare(P, da.F32, 300, 16, 16, P, pb - 1, None), ENOMEM, b"planes buffer too small")
    failed(lib.dbgsom_filter_prepare(P, da.F32, 300, 16, 16, P + 64, pb, None), EINVAL, b"bad pointer")
    failed(lib.dbgsom_filter_prepare(P, da.F32, 300, 16, 15, P, pb, None), EINVAL, b"bad samples")
    host = np.zeros(8, dtype=np.uint32)
    failed(lib.dbgsom_bmu_filtered_counts(P, 300, 16, 130, host.ctypes.data, 2, None), EINVAL, b"n_counts")
    failed(lib.dbgsom_bmu_filtered_counts(P, 300, 16, 130, host.ctypes.data, 4, None), EINVAL, b"n_counts")
    gap = np.zeros(4, dtype=np.float32)
    failed(lib.dbgsom_bmu_filtered_gaps(P, 300, 16, 8193, gap.ctypes.data, None), EINVAL, b"8192")
    failed(lib.dbgsom_bmu_filtered_gaps(None, 300, 16, 130, gap.ctypes.data, None), EINVAL, b"null pointer")
    failed(lib.dbgsom_bmu_filtered_gaps(P, 300, 16, 130, None, None), EINVAL, b"null pointer")
    assert lib.dbgsom_bmu_filtered_workspace_bytes(0, 16, 130) == 0
