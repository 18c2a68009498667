"""No GPU: the cases of tests/epoch_tail.py have the properties their names claim, the golden file holds every one of
them, and the workspace-size functions of the library still cover what the kernels' layouts take (the formulas of
accumulate.hip and smooth.hip restated)."""
import numpy as np
import pytest

from tests import device_abi as da
from tests import epoch_tail as et


def _align(x, a=256):
    return (x + a - 1) // a * a


# ---- the sort cases -----------------------------------------------------------------------------------------------------
def test_sort_shapes_hold_what_the_issue_names():
    assert set(et.SORT_N) == {1, 63, 64, 65, 511, 512, 513, 2047, 2049, 300000, 300001}
    assert da.hs_for(300000) == 512 and da.hs_for(300001) == 2048           # the first N of the 2048-sample form
    assert {1, 2, 33, 1024} < set(et.SORT_M)
    # the four-wavefront scatter keeps 4 counters of 4 bytes per neuron in LDS; two workgroups must fit a CU's 160 KB
    assert 2 * 16 * et.SCATTER4_MAX_M <= 160 * 1024 < 2 * 16 * (et.SCATTER4_MAX_M + 1)
    assert et.SCATTER4_MAX_M in et.SORT_M and et.SCATTER4_MAX_M + 1 in et.SORT_M
    assert max(et.SORT_M) <= da.MAX_PROTOTYPES
    assert set(et.SORT_SHAPES) == {(N, M) for N in et.SORT_N for M in et.SORT_M}
    assert len({(-(-N // da.hs_for(N))) for N in et.SORT_N}) >= 6                # one workgroup .. hundreds


@pytest.mark.parametrize("N,M", [(1, 1), (65, 2), (513, 33), (2049, 1024), (300001, et.SCATTER4_MAX_M + 1)])
def test_sort_winner_kinds_are_what_they_are_called(N, M):
    for kind in et.SORT_KINDS:
        w = et.sort_winners(kind, N, M)
        assert w.dtype == np.int64 and w.shape == (N,)
        assert np.array_equal(w, et.sort_winners(kind, N, M))                   # fixed seeds
        inside = (w >= 0) & (w < M)
        if kind == "mixed_bad":
            assert (w == -1).any() and (N == 1 or (w == M).any()) and set(w[~inside]) <= {-1, M}
            assert N <= 2 or inside.any()
        else:
            assert inside.all()
    assert len(set(et.sort_winners("equal", N, M))) == 1
    assert np.array_equal(et.sort_winners("modulo", N, M), np.arange(N) % M)
    desc = et.sort_winners("descending", N, M)
    assert (np.diff(desc) <= 0).all()
    if N >= 2049 and M >= 33:
        counts = np.bincount(et.sort_winners("skewed", N, M), minlength=M)
        assert counts[0] > 4 * N // M and len(set(desc)) > 1                    # a heavy head


# ---- the smoothing cases ------------------------------------------------------------------------------------------------
def test_smooth_cases_hold_what_the_issue_names():
    assert set(et.SMOOTH_CASES) == {(1, 2), (5, 6), (17, 64), (130, 66), (257, 130), (1030, 2)}
    for (M, d), splits in et.SMOOTH_CASES.items():
        assert da.gemm_splits(M, d) == splits
        assert d % 2 == 0                                                       # the LDS-DMA product kernel
    assert et.SMOOTH_CASES[(257, 130)] == 4 and et.SMOOTH_CASES[(17, 64)] == 1
    assert any(M > 1024 for M, _ in et.SMOOTH_CASES)                            # second trip of the 1024-leaf tree
    assert any(d > 64 and d % 64 for _, d in et.SMOOTH_CASES)                   # a partial last trip over the columns
    (M1, d1), (M2, d2) = et.SMOOTH_TWICE
    assert M1 > M2 and (M1, d1) in et.SMOOTH_CASES and (M2, d2) in et.SMOOTH_CASES
    assert et.SMOOTH_NAN_CASE in et.SMOOTH_CASES


@pytest.mark.parametrize("M,d", sorted(et.SMOOTH_CASES))
def test_smooth_inputs_have_dead_neurons_and_fixed_seeds(M, d):
    S, K, a, E, hop, W_old = et.smooth_case(M, d)
    again = et.smooth_case(M, d)
    assert all(np.array_equal(x, y) for x, y in zip((S, K, a, E, hop, W_old), again))
    assert S.shape == (M, d) and W_old.shape == (M, d) and hop.shape == (M, M)
    assert (a > 0).any()
    if M > 3:
        assert (a == 0).any()
    assert (K[a == 0] == 0).all() and (S[a == 0] == 0).all()
    # every row reaches a live neuron with a weight that does not underflow: no NaN row in these cases
    g = np.exp(-(hop.astype(np.float64) ** 2) / (2 * et.SIGMA ** 2)) * a[None, :]
    assert (g.sum(axis=1) > 0).all()


def test_smooth_nan_case_has_a_row_whose_every_weight_is_zero():
    S, K, a, E, hop, W_old = et.smooth_case(*et.SMOOTH_NAN_CASE, nan_row=True)
    g = np.exp(-(hop.astype(np.float64) ** 2) / (2 * et.SIGMA ** 2)) * a[None, :]
    assert (g.sum(axis=1) == 0).sum() == 1


def test_epoch_inputs_are_fixed():
    X, W, hop, gamma = et.epoch_inputs()
    N, d, rows, cols = et.EPOCH_SHAPE
    assert (N, d, rows * cols) == (4096, 16, 64)
    assert X.shape == (N, d) and X.dtype == np.float32 and W.shape == (64, d) and hop.shape == (64, 64)
    X2, W2, hop2, gamma2 = et.epoch_inputs()
    assert np.array_equal(X, X2) and np.array_equal(W, W2) and gamma == gamma2


# ---- the golden file ----------------------------------------------------------------------------------------------------
def test_golden_file_holds_every_case():
    import os

    assert os.path.getsize(et.GOLDEN) < 1_000_000
    with np.load(et.GOLDEN) as z:
        assert sorted(z.files) == sorted(et.golden_keys())
        for (M, d) in et.SMOOTH_CASES:
            for layout in et.LAYOUTS:
                k = et.smooth_key(M, d, layout)
                assert z[k + "_W"].shape == (M, d) and z[k + "_W"].dtype == np.float64
                assert z[k + "_chg"].shape == (1,) and np.isfinite(z[k + "_W"]).all() and np.isfinite(z[k + "_chg"]).all()
        for layout in et.LAYOUTS:
            k = et.smooth_key(*et.SMOOTH_NAN_CASE, layout, nan_row=True)
            assert np.isnan(z[k + "_W"]).any(axis=1).sum() == 1 and np.isnan(z[k + "_chg"]).all()
        N, d, rows, cols = et.EPOCH_SHAPE
        assert z["epoch_W"].shape == (rows * cols, d) and z["epoch_activations"].sum() == N
        assert z["epoch_errors"].shape == (rows * cols,) and z["epoch_change_total"].shape == (1,)


# ---- workspace sizes ----------------------------------------------------------------------------------------------------
def _accumulate_layout_bytes(N, d, M, ns):
    """what accumulate.hip's carve takes: order, block histograms, count, seg_start, chunk_pre, chunk slab, group slab,
    ticket, the histogram workgroups' out-of-range flags"""
    hs = da.hs_for(N)
    nb = -(-N // hs)
    maxchunks = -(-N // da.CH) + M
    parts = [N * 4, nb * M * 4, M * 4, (M + 1) * 4, (M + 1) * 4, maxchunks * (d + ns) * 8,
             M * da.finalize_groups(M) * (d + ns) * 8, 256, nb * 4]
    return sum(_align(p) for p in parts)


def _smooth_layout_bytes(M, d):
    """what smooth.hip's carve_smooth takes: C (padded rows + a tile of slack), G, den, the row changes, split-K pieces"""
    Mp = (M + 15) // 16 * 16
    ks = da.gemm_splits(M, d)
    parts = [(Mp * d + 64) * 8, (M * Mp + 16) * 8, M * 8, M * 8, ks * M * d * 8 if ks > 1 else 0]
    return sum(_align(p) for p in parts)


@pytest.fixture(scope="module")
def lib():
    from dbgsom_amd import _native

    return _native.load()


@pytest.mark.parametrize("N,M", [(1, 1), (513, 33), (2049, 1024), (300000, 2), (300001, et.SCATTER4_MAX_M + 1),
                                 (1_000_000, 1024), (60_000, 506)])
def test_accumulate_workspace_covers_the_layout(lib, N, M):
    for d in (et.SORT_D, 784):
        assert lib.dbgsom_accumulate_workspace_bytes(N, d, M) >= _accumulate_layout_bytes(N, d, M, 2)
        assert lib.dbgsom_accumulate_weighted_workspace_bytes(N, d, M) >= _accumulate_layout_bytes(N, d, M, 3)
        # the order comes first: N int32 fit in front of everything else
        assert lib.dbgsom_accumulate_workspace_bytes(N, d, M) >= _align(4 * N) + 4 * (-(-N // da.hs_for(N))) * (M + 1)


@pytest.mark.parametrize("M,d", sorted(et.SMOOTH_CASES) + [(1024, 784), (2025, 128)])
def test_smooth_workspace_covers_the_layout(lib, M, d):
    assert lib.dbgsom_smooth_workspace_bytes(M, d) >= _smooth_layout_bytes(M, d)
