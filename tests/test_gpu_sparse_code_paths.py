"""Sparse coding on the MI355X (csrc/sparse_code.hip), the paths that data must reach: both overflow
passes, the cap boundaries 64 and 192, the max_iter stop, slot reuse, and the edge shapes of the GEMMs and
of the class-probability epilogue -- against scikit-learn's lars_path_gram row by row
(tests/sparse_code_inputs.py), codes and iteration counters.

The inputs are planted (tests/sparse_code_inputs.py); tests/test_sparse_code_inputs_cpu.py proves on the
CPU that scikit-learn raises no warning on them, that their supports land in the intended pass and that
scikit-learn moves against itself by at most 1/100 of the gates below.

Gates (DESIGN.md 4b "Parity rule"): max |dcode| <= 1e-10 for float64 queries, <= 1e-6 for float32
queries; predict_proba rtol 1e-9 (float32 queries 1e-5), atol 1e-12."""
import warnings

import numpy as np
import pytest

from tests import sparse_code_inputs as si

pytestmark = pytest.mark.gpu

DTYPES = ("float64", "float32")
PROBA_RTOL = {"float64": 1e-9, "float32": 1e-5}

# csrc/sparse_code.hip: slot_doubles(), SC_SLOT_BUDGET and the 4096 cap of carve_ws
SC_SLOT_BUDGET = (256 << 20, 32 << 20)


def slot_doubles(cap):
    return cap * (cap + 3) // 2 + 3 * (cap + 1) + 3 * (2 * cap + 2) + (5 * cap + 6) // 2


def n_slots(which, M, max_iter, rows):
    cap = max(1, min(M, max_iter))
    if which == 0:
        cap = min(cap, si.SC_CAP1)
    return max(1, min(4096, SC_SLOT_BUDGET[which] // (8 * slot_doubles(cap)), max(rows, 1)))


@pytest.fixture(scope="module")
def hip():
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0)
    yield be
    be.release()


def _run(hip, W, X, **kw):
    """One device call in which any warning is an error; returns (result, counters)."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = hip.sparse_code(W, X, **kw)
    return out, dict(hip.sparse_code_counts)


def _max_err(got, ref):
    assert got.shape == ref.shape
    return float(np.abs(got - ref).max()) if got.size else 0.0


def _check_codes(tag, got, ref, dtype):
    err = _max_err(got, ref)
    print("%s %s: max |dcode| = %.3e" % (tag, dtype, err))
    assert err <= si.GATE[np.dtype(dtype)], "max |dcode| = %.3e" % err
    return err


def _check_counters(tag, cnt, iters, rows):
    print("%s counters: %s" % (tag, cnt))
    assert cnt["samples"] == rows
    assert cnt["iterations"] == int(iters.sum())
    assert cnt["max_iterations"] == int(iters.max())
    assert cnt["degenerate"] == 0 and cnt["early_stops"] == 0


def _proba_ref(code, P):
    raw = code @ P
    with np.errstate(invalid="ignore", divide="ignore"):
        return raw / raw.sum(axis=1)[:, None]


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_overflow_pass_reached_by_data(hip, dtype):
    W, _, _ = si.case("pass1")
    X, _ = si.case_queries("pass1", dtype)
    rows = X.shape[0]
    assert rows >= 64
    ref, iters = si.case_reference("pass1", dtype)
    got, cnt = _run(hip, W, X)
    _check_codes("pass1", got, ref, dtype)
    _check_counters("pass1", cnt, iters, rows)
    assert cnt["overflow"] == rows
    assert si.SC_CAP < cnt["max_active"] <= si.SC_CAP1
    assert cnt["max_active"] >= np.count_nonzero(ref, axis=1).max()
    assert cnt["drops"] > 0
    # the epilogue out of a global slot
    P = np.abs(np.random.default_rng(11).normal(size=(W.shape[0], 70)))
    pr, _ = _run(hip, W, X, P=P)
    np.testing.assert_allclose(pr, _proba_ref(ref, P), rtol=PROBA_RTOL[dtype], atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_overflow_pass_reached_by_data_in_a_mixed_call(hip, dtype):
    """Rows for the LDS path, the first and the second pass in one call, shuffled.  The second pass has
    32 MiB / (8 * slot_doubles(400) = 681 696 B) = 49 slots at M = 400: the 64 rows it takes in float64
    make every slot serve a second row."""
    W, _, _ = si.case("pass2")
    X, kind = si.case_queries("pass2", dtype)
    rows, M = X.shape[0], W.shape[0]
    ref, iters = si.case_reference("pass2", dtype)
    support = np.count_nonzero(ref, axis=1)
    second = int((support > si.SC_CAP1).sum())
    if dtype == "float64":
        assert n_slots(1, M, 1000, rows) == 49 and second >= 64 > n_slots(1, M, 1000, rows)
    got, cnt = _run(hip, W, X)
    _check_codes("pass2 (mixed)", got, ref, dtype)
    _check_counters("pass2 (mixed)", cnt, iters, rows)
    assert cnt["overflow"] == int((kind != 5).sum()) and 0 < cnt["overflow"] < rows
    assert si.SC_CAP1 < support.max() <= cnt["max_active"] <= M
    assert cnt["drops"] > 0
    # the rows of each kind came back in their own positions
    for s in np.unique(kind):
        assert _max_err(got[kind == s], ref[kind == s]) <= si.GATE[np.dtype(dtype)]
    if dtype == "float64":
        # every row of the mixed call equals the same row coded alone
        for i in range(rows):
            alone, c1 = _run(hip, W, X[i:i + 1])
            assert c1["iterations"] == iters[i]
            assert np.array_equal(alone[0], got[i]), "row %d (s = %d)" % (i, kind[i])


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_overflow_pass_with_large_slots(hip, dtype):
    """784 x 1030: slots of cap min(M, max_iter) = 1000 (4 104 096 B each, 8 of them in 32 MiB), paths of up
    to ~870 iterations, close to max_iter."""
    W, _, _ = si.case("pass2_big")
    X, _ = si.case_queries("pass2_big", dtype)
    rows, M = X.shape[0], W.shape[0]
    ref, iters = si.case_reference("pass2_big", dtype)
    if dtype == "float64":
        assert n_slots(1, M, 1000, rows) == 8 and rows >= 16
    assert 700 < iters.max() < 1000
    got, cnt = _run(hip, W, X)
    _check_codes("pass2_big", got, ref, dtype)
    _check_counters("pass2_big", cnt, iters, rows)
    assert cnt["overflow"] == rows
    assert si.SC_CAP1 < np.count_nonzero(ref, axis=1).max() <= cnt["max_active"] <= 1000
    assert cnt["drops"] > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", sorted(si.BOUNDARY))
def test_all_prototypes_active_at_the_cap_boundaries(hip, M, dtype):
    name = "all_active_%d" % M
    W, _, _ = si.case(name)
    X, _ = si.case_queries(name, dtype)
    assert W.shape == (M, M + 3)
    ref, iters = si.case_reference(name, dtype)
    assert (np.count_nonzero(ref, axis=1) == M).all()
    got, cnt = _run(hip, W, X)
    _check_codes(name, got, ref, dtype)
    _check_counters(name, cnt, iters, X.shape[0])
    assert cnt["max_active"] == M
    assert cnt["overflow"] == (0 if M <= si.SC_CAP else X.shape[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_map_with_support_below_d(hip, dtype):
    """M = 200 > d = 64, planted with s = 10: the support stays well below d (a support that reaches d is
    ill conditioned, see sparse_code_inputs.sweep_shapes)."""
    W, _, _ = si.case("wide")
    X, _ = si.case_queries("wide", dtype)
    ref, iters = si.case_reference("wide", dtype)
    got, cnt = _run(hip, W, X)
    _check_codes("wide", got, ref, dtype)
    _check_counters("wide", cnt, iters, X.shape[0])
    assert cnt["overflow"] == 0 and cnt["drops"] > 0
    assert np.count_nonzero(ref, axis=1).max() <= cnt["max_active"] <= si.SC_CAP


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("max_iter", si.MAX_ITERS)
def test_max_iter_stops_the_path(hip, max_iter, dtype):
    W, _, _ = si.case("pass1")
    X, _ = si.case_queries("pass1", dtype)
    X = X[:si.MAX_ITER_ROWS]
    ref, iters = si.case_reference("pass1", dtype, max_iter, si.MAX_ITER_ROWS)
    got, cnt = _run(hip, W, X, max_iter=max_iter)
    _check_codes("max_iter=%d" % max_iter, got, ref, dtype)
    _check_counters("max_iter=%d" % max_iter, cnt, iters, X.shape[0])
    assert cnt["max_iterations"] == max_iter
    assert cnt["max_active"] <= max_iter
    P = np.abs(np.random.default_rng(12).normal(size=(W.shape[0], 10)))
    pr, _ = _run(hip, W, X, P=P, max_iter=max_iter)
    if max_iter == 0:
        assert not got.any()
        assert np.isnan(pr).all()   # 0 / 0, as for a zero row
    else:
        np.testing.assert_allclose(pr, _proba_ref(ref, P), rtol=PROBA_RTOL[dtype], atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", si.sweep_shapes(), ids=lambda t: "x".join(map(str, t)))
def test_gemm_and_epilogue_shapes(hip, shape, dtype):
    W, X = si.sweep_case(*shape)
    X = si.queries(X, dtype)
    assert X.flags.c_contiguous and W.flags.c_contiguous and X.dtype == np.dtype(dtype)
    ref, iters = si.reference(W, X)
    got, cnt = _run(hip, W, X)
    _check_codes("%dx%dx%d" % shape, got, ref, dtype)
    _check_counters("%dx%dx%d" % shape, cnt, iters, X.shape[0])
    assert cnt["overflow"] == 0
    for C in si.SWEEP_C:
        P = np.abs(np.random.default_rng(C).normal(size=(W.shape[0], C)))
        pr, _ = _run(hip, W, X, P=P)
        assert pr.shape == (X.shape[0], C)
        np.testing.assert_allclose(pr, _proba_ref(ref, P), rtol=PROBA_RTOL[dtype], atol=1e-12)


def test_overflow_passes_do_not_depend_on_chunks_caps_or_earlier_calls(hip):
    """On the mixed second-pass case: chunks of 7 rows (fewer than the slots, a multiple of nothing), the
    LDS cap at 1 and 64, and the same call twice on the reused workspace give the same bits."""
    W, _, _ = si.case("pass2")
    X, _ = si.case_queries("pass2", "float64")
    base, cnt = _run(hip, W, X)
    assert cnt["max_active"] > si.SC_CAP1
    again, cnt2 = _run(hip, W, X)
    assert np.array_equal(again, base) and cnt2 == cnt
    old_chunk, old_cap = hip.sc_chunk_rows, hip.sc_cap
    try:
        hip.sc_chunk_rows = 7
        chunked, cnt7 = _run(hip, W, X)
        assert np.array_equal(chunked, base)
        assert cnt7["iterations"] == cnt["iterations"] and cnt7["overflow"] == cnt["overflow"]
        hip.sc_chunk_rows = old_chunk
        for cap in (1, 64):
            hip.sc_cap = cap
            capped, cntc = _run(hip, W, X)
            assert np.array_equal(capped, base), "sc_cap = %d" % cap
            assert cntc["iterations"] == cnt["iterations"]
            assert cntc["overflow"] == (X.shape[0] if cap == 1 else cnt["overflow"])
    finally:
        hip.sc_chunk_rows = old_chunk
        hip.sc_cap = old_cap
