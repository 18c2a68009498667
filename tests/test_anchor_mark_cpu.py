"""CPU: the candidate rule of anchor_mark_kernel (csrc/filter.hip 2f) as tests/anchor_mark.py restates it in NumPy, with
the code's margins: whatever it rules out for a workgroup is at least 2 rho_i further (squared) from every sample of the
workgroup than the sample's nearest prototype -- so every all-pairs winner and every tie partner survives.  Random
blobs, and the cases built to sit on the rule's edges: exact ties, duplicated prototypes, a sample equal to its anchor,
an anchor equal to a prototype, runs of radius 0.  The radii are taken at the LEAST the device may store (the exact
radius, rounded down), the bounds as the kernel forms them in float64."""
import numpy as np
import pytest

from tests import anchor_mark as am


def _least_R(table):
    with np.errstate(invalid="ignore"):
        r = np.sqrt(table["R2"]).astype(np.float64)
    return np.where(np.isfinite(r), np.nextafter(r, 0.0), np.inf)


def _check(X, W, A, min_ruled_out=None):
    N, d = X.shape
    M = W.shape[0]
    anchors, aof, order = am.buckets(X, A)
    table = am.run_table(X, anchors, aof, order)
    low, up, seed, yy_max = am.bounds(anchors, W)
    lists = am.rule_lists(_least_R(table), table, low, up, seed, yy_max, M, d)
    need = am.group_sets(am.must_keep(X, W), order)
    assert len(lists) == len(need) == (N + 127) // 128
    for g, (have, must) in enumerate(zip(lists, need)):
        missing = np.setdiff1d(must, have)
        assert missing.size == 0, (g, missing[:8])
    mean = float(np.mean([len(h) for h in lists]))
    if min_ruled_out is not None:      # (the case tests something: the rule does rule prototypes out)
        assert M - mean >= min_ruled_out, mean
    return lists, table, seed


@pytest.mark.parametrize("N,d,M,A,radii", [(1000, 16, 130, 256, 8.0), (1000, 70, 256, 256, 8.0), (700, 320, 130, 64, 8.0),
                                           (1000, 70, 256, 256, 2.5), (300, 16, 130, 17, 4.0), (200, 70, 130, 256, 8.0)])
def test_random_blobs(N, d, M, A, radii):
    X, W = am.blobs(N, d, M, "cpu", radii=radii)
    # (well separated clusters: the case tests something only if the rule rules out a good part of the map; every row
    #  its own anchor, N = 200, leaves the workgroups in sample order -- all clusters mixed -- and rules out less)
    lists, _, _ = _check(X, W, A, min_ruled_out=M / 4 if radii >= 8.0 else None)
    print(f"N={N} d={d} M={M} A={A} radii={radii}: mean list {np.mean([len(h) for h in lists]):.1f}")


def test_exact_ties_and_duplicated_prototypes():
    X, W = am.blobs(600, 48, 130, "ties")
    W[[5, 70, 129]] = W[5]                       # three copies of one row ...
    W[[11, 12]] = X[40].astype(np.float64)       # ... two copies of a sample (distance 0 to it, twice)
    X[300] = X[40]
    lists, table, seed = _check(X, W, 64, min_ruled_out=40)
    keep = am.must_keep(X, W)
    assert keep[40, 11] and keep[40, 12] and keep[300, 11] and keep[300, 12]
    r = am.exact_r(X, W)
    near5 = np.flatnonzero(r.argmin(axis=1) == 5)
    assert near5.size and keep[near5][:, [5, 70, 129]].all()


def test_a_sample_equal_to_its_anchor_and_an_anchor_equal_to_a_prototype():
    X, W = am.blobs(512, 32, 130, "equal")
    anchors, aof, order = am.buckets(X, 32)
    for k in range(32):                          # every anchor row sits in its own bucket, at distance 0
        assert (X[aof == k].astype(np.float64) == anchors[k]).all(axis=1).any()
    W[7] = anchors[3]                            # U[3] is then rho alone
    W[8] = anchors[3]
    lists, table, seed = _check(X, W, 32, min_ruled_out=40)
    assert seed[3] == 7                          # (the lower of the two copies)
    low, up, _, _ = am.bounds(anchors, W)
    assert low[3, 7] == 0 and low[3, 8] == 0 and 0 < up[3] < 1e-5


def test_runs_of_radius_zero():
    """every row its own anchor (N < 256), and a sample set of 40 distinct rows repeated: R = 0 in every run"""
    X, W = am.blobs(200, 16, 130, "r0")
    _, table, _ = _check(X, W, 256)
    assert not table["R2"].any() and len(table["anchor"]) == 200 and table["run_start"][1] == 128
    base, W = am.blobs(130, 16, 130, "r0rep")
    X = np.ascontiguousarray(np.repeat(base[:4], 100, axis=0))   # anchors: rows 0, 100, 200, 300 -- the four rows
    lists, table, _ = _check(X, W, 4, min_ruled_out=60)
    assert not table["R2"].any() and len(table["anchor"]) == 4 + 3


def test_rows_that_are_not_finite_leave_the_whole_map():
    X, W = am.blobs(300, 16, 130, "nan")
    X[17, 3] = np.nan
    anchors, aof, order = am.buckets(X, 16)
    table = am.run_table(X, anchors, aof, order)
    low, up, seed, yy_max = am.bounds(anchors, W)
    lists = am.rule_lists(_least_R(table), table, low, up, seed, yy_max, 130, 16)
    g = int(np.flatnonzero(order == 17)[0]) // 128
    assert len(lists[g]) == 130 and min(len(h) for h in lists) < 130
    W[5] = np.nan                                # a NaN prototype: no bound, kept everywhere; the others as before
    low2, up2, seed2, yy2 = am.bounds(anchors, W)
    assert not low2[:, 5].any() and (seed2 != 5).all() and np.isfinite(yy2)
    lists2 = am.rule_lists(_least_R(table), table, low2, up2, seed2, yy2, 130, 16)
    assert all(5 in h for h in lists2)
    W[6, 2] = np.inf                             # an infinite one: max |w|^2 is, and nothing is ruled out anywhere
    low3, up3, seed3, yy3 = am.bounds(anchors, W)
    lists3 = am.rule_lists(_least_R(table), table, low3, up3, seed3, yy3, 130, 16)
    assert all(len(h) == 130 for h in lists3)
