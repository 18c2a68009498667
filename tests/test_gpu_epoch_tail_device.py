"""MI355X: the kernels behind the exact stage of an epoch -- the counting sort of dbgsom_accumulate (histogram,
column scan, scatter in its four-wavefront and one-wavefront forms, the status word stored by the scan), the
smoothing (dbgsom_smooth: operand kernel, split-K pieces, row changes, change_total) and one whole dbgsom_ctx_epoch.

The sort is checked against NumPy exactly (stable order, counts, status); W', change_total and the epoch's results are
compared BIT FOR BIT with tests/golden/epoch_tail_parent.npz, which tools/record_epoch_tail_golden.py recorded from
the library of the commit in front of the batched tail kernels.  Cases: tests/epoch_tail.py."""
import numpy as np
import pytest

from tests import device_abi as da
from tests import epoch_tail as et

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


@pytest.fixture(scope="module")
def golden():
    with np.load(et.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- the counting sort ------------------------------------------------------------------------------------------------
class _Sort:
    """one (N, M): rows, workspace and outputs staged once, dbgsom_accumulate called per winner vector"""

    def __init__(self, nat, N, M):
        import torch

        self.nat, self.N, self.M, self.torch = nat, N, M, torch
        X, kw, dist = et.sort_rows(N)
        self.x_t, self.xptr = da.stage(X, et.SORT_D, 0, "f32")
        self.kw_t, self.dist_t = da.dev(kw), da.dev(dist)
        self.nbytes = nat.load().dbgsom_accumulate_workspace_bytes(N, et.SORT_D, M)
        assert self.nbytes > 0
        self.ws_t, self.ws = da.workspace(self.nbytes)

    def call(self, winners, status=True):
        """-> (order: the first N int32 of the workspace, a, status word or None)"""
        torch, N, M, d = self.torch, self.N, self.M, et.SORT_D
        win_t = da.dev(winners)
        sums = torch.full((M * (d + 3),), float("nan"), dtype=torch.float64, device="cuda")
        st = torch.full((1,), 77, dtype=torch.int32, device="cuda") if status else None
        self.nat.call("dbgsom_accumulate", self.xptr, da.F32, N, d, d, win_t.data_ptr(), self.kw_t.data_ptr(),
                      self.dist_t.data_ptr(), M, sums.data_ptr(), st.data_ptr() if status else None, self.ws,
                      self.nbytes, da.stream())
        torch.cuda.synchronize()
        skip = self.ws - self.ws_t.data_ptr()
        order = self.ws_t[skip:skip + 4 * N].cpu().numpy().view(np.int32)
        a = sums[M * d + M:M * d + 2 * M].cpu().numpy()
        return order, a, (int(st.cpu()[0]) if status else None)

    def check(self, winners, status=True):
        order, a, st = self.call(winners, status)
        inside = (winners >= 0) & (winners < self.M)
        rows = np.flatnonzero(inside)
        want = rows[np.argsort(winners[rows], kind="stable")]          # stable by (winner, row) over the rows in range
        assert np.array_equal(order[:rows.size], want)
        assert np.array_equal(a, np.bincount(winners[rows], minlength=self.M))
        if status:
            assert st == (0 if inside.all() else 1)                    # stored, whatever the word held before


@pytest.mark.parametrize("N,M", et.SORT_SHAPES)
def test_sort_is_the_stable_order_with_counts_and_status(nat, N, M):
    s = _Sort(nat, N, M)
    for kind in et.SORT_KINDS:
        w = et.sort_winners(kind, N, M)
        assert (((w < 0) | (w >= M)).any()) == (kind == "mixed_bad")
        s.check(w)


@pytest.mark.parametrize("N,M", [(513, 33), (2049, et.SCATTER4_MAX_M + 1), (300001, 1024)])
def test_sort_status_belongs_to_its_call_and_may_be_null(nat, N, M):
    """two calls in a row on ONE workspace, bad winners first and the other way round: each call its own status (the
    word pre-filled with 77 each time); status_dev = NULL works on both kinds"""
    s = _Sort(nat, N, M)
    bad, clean = et.sort_winners("mixed_bad", N, M), et.sort_winners("skewed", N, M)
    for first, second in ((bad, clean), (clean, bad)):
        s.check(first)
        s.check(second)
    s.check(bad, status=False)
    s.check(clean, status=False)
    s.check(clean)


# ---- dbgsom_smooth ----------------------------------------------------------------------------------------------------
def _check_smooth(nat, golden, M, d, nan_row, ws=None):
    case = et.smooth_case(M, d, nan_row)
    for layout in et.LAYOUTS:
        W, chg = et.smooth_call(nat, case, layout, ws)
        key = et.smooth_key(M, d, layout, nan_row)
        assert np.isnan(W).any() == nan_row and np.isnan(chg).any() == nan_row
        assert _same_bits(W, golden[key + "_W"]), key
        assert _same_bits(chg, golden[key + "_chg"]), key


@pytest.mark.parametrize("M,d", sorted(et.SMOOTH_CASES))
def test_smooth_is_the_parent_bit_for_bit(nat, golden, M, d):
    assert da.gemm_splits(M, d) == et.SMOOTH_CASES[(M, d)]
    _check_smooth(nat, golden, M, d, nan_row=False)


def test_smooth_with_a_row_of_zero_weights_is_the_parent_bit_for_bit(nat, golden):
    _check_smooth(nat, golden, *et.SMOOTH_NAN_CASE, nan_row=True)


def test_smooth_twice_on_one_workspace_larger_map_first(nat, golden):
    (M1, d1), (M2, d2) = et.SMOOTH_TWICE
    lib = nat.load()
    nbytes = max(lib.dbgsom_smooth_workspace_bytes(M1, d1), lib.dbgsom_smooth_workspace_bytes(M2, d2))
    ws_t, ptr = da.workspace(nbytes)
    _check_smooth(nat, golden, M1, d1, False, (ws_t, ptr, nbytes))
    _check_smooth(nat, golden, M2, d2, False, (ws_t, ptr, nbytes))


# ---- one epoch through the context ------------------------------------------------------------------------------------
def test_epoch_is_the_parent_bit_for_bit(nat, golden):
    got = et.epoch_call(nat)
    for key in et.EPOCH_KEYS:
        assert _same_bits(got[key], golden[key]), key
    assert got["epoch_activations"].sum() == et.EPOCH_SHAPE[0]
