"""MI355X: queries on rows with missing entries (csrc/masked.hip) against the NumPy oracle of
tests/test_missing_cpu.py -- distances to rtol 1e-12 (derived there), winners exactly, with no row left out --
exact zeros and ties, independence of the batch, the fill, and the estimators' NaN-aware queries."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from tests import golden_inputs as gi
from tests.test_missing_cpu import (DTYPES, GAP, GRID, GRID_IDS, RTOL, case, fill_numpy, masked_bmu, masked_distances,
                                    punch, smallest_gap, winners_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from dbgsom_amd.backend import HipBackend

    return HipBackend(0)


def _check_against_oracle(got, D, k):
    dist, idx = got
    want_dist, want_idx = winners_of(D, k)
    assert idx.dtype == np.int64 and dist.dtype == np.float64 and idx.shape == want_idx.shape
    err = float(np.max(np.abs(dist - want_dist) / np.where(want_dist > 0, want_dist, 1.0)))
    print(f"k = {k}: largest relative distance difference {err:.2e}")
    assert np.array_equal(idx, want_idx)                       # every row
    np.testing.assert_allclose(dist, want_dist, rtol=RTOL, atol=0)


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,M,frac,dt", GRID, ids=GRID_IDS)
def test_backend_matches_the_oracle(be, N, d, M, frac, dt):
    X, W, D = case(N, d, M, frac, np.dtype(dt).name)
    assert smallest_gap(D) > GAP
    for k in (1, 2):
        if M >= k:
            _check_against_oracle(be.bmu_masked(W, k, X), D, k)


def _device_call(X, W, k, pad=0, fill=False):
    """dbgsom_bmu_masked (and dbgsom_fill_missing) on torch tensors; rows padded by `pad` columns of junk."""
    import torch

    from dbgsom_amd import _native

    N, d = X.shape
    M = W.shape[0]
    Xp = np.full((N, d + pad), 7.0, dtype=X.dtype)
    Xp[:, :d] = X
    code = _native.F32 if X.dtype == np.float32 else _native.F64
    Xt, Wt = torch.from_numpy(Xp).cuda(), torch.from_numpy(np.ascontiguousarray(W)).cuda()
    idx = torch.empty((N, k), dtype=torch.int64, device="cuda")
    dist = torch.empty((N, k), dtype=torch.float64, device="cuda")
    nbytes = _native.load().dbgsom_bmu_masked_workspace_bytes(code, N, d, M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.call("dbgsom_bmu_masked", Xt.data_ptr(), code, N, d, d + pad, Wt.data_ptr(), M, d, k, idx.data_ptr(),
                 dist.data_ptr(), ws.data_ptr(), nbytes, stream)
    if fill:
        _native.call("dbgsom_fill_missing", Xt.data_ptr(), code, N, d, d + pad, Wt.data_ptr(), M, d, idx.data_ptr(), k,
                     stream)
    torch.cuda.synchronize()
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    if k == 1:
        dist, idx = dist.reshape(-1), idx.reshape(-1)
    return dist, idx, Xt.cpu().numpy()


@pytest.mark.parametrize("N,d,M,pad", [(257, 17, 5, 3), (1000, 130, 300, 0)])
@pytest.mark.parametrize("dt", DTYPES)
def test_device_level_call_matches_the_oracle(N, d, M, pad, dt):
    X, W, D = case(N, d, M, 0.3, np.dtype(dt).name)
    for k in (1, 2):
        dist, idx, Xf = _device_call(X, W, k, pad=pad, fill=True)
        _check_against_oracle((dist, idx), D, k)
        assert np.array_equal(Xf[:, :d], fill_numpy(X, W, idx)) and (Xf[:, d:] == 7.0).all()


def test_many_rows_take_the_wide_kernel_with_the_same_bits(be):
    """8192 rows and more go through the kernel that walks 16 rows per workgroup instead of 4: the bits of a row
    do not depend on it (the small batches below are checked against the oracle above)."""
    for (N, d, M, reps) in [(257, 17, 5, 32), (1000, 130, 300, 9)]:
        for dt in DTYPES:
            X, W, D = case(N, d, M, 0.3, np.dtype(dt).name)
            big = np.tile(X, (reps, 1))
            assert big.shape[0] >= 8192
            for k in (1, 2):
                dist, idx = be.bmu_masked(W, k, big)
                small = be.bmu_masked(W, k, X)
                _check_against_oracle(small, D, k)
                assert np.array_equal(idx, np.concatenate([small[1]] * reps))
                assert np.array_equal(dist, np.concatenate([small[0]] * reps))


# ---- 2. zero and ties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,d", [(12, 20), (300, 33)])
def test_exact_zero_and_ties_to_the_lower_index(be, dt, M, d):
    rng = np.random.default_rng(M + d)
    W = (3.0 * rng.standard_normal((M, d))).astype(dt).astype(np.float64)   # (float32: W made from the cast values)
    W[7], W[M - 1] = W[3], W[0]
    rows, first, second = [], [], []
    for (lo, hi) in ((3, 7), (0, M - 1)):
        for src in (lo, hi):
            for frac in (0.0, 0.3, 0.9):
                rows.append(punch(W[src][None, :].astype(dt), frac, 10 * src + int(10 * frac))[0])
                first.append(lo)
                second.append(hi)
    X = np.array(rows, dtype=dt)
    assert np.isnan(X).any()
    dist, idx = be.bmu_masked(W, 1, X)
    assert (dist == 0.0).all() and np.array_equal(idx, first)
    dist, idx = be.bmu_masked(W, 2, X)
    assert (dist == 0.0).all() and np.array_equal(idx[:, 0], first) and np.array_equal(idx[:, 1], second)
    # two bit-identical prototypes get bit-identical distances, wherever they stand
    far = punch((W[5][None, :] + 1.0).astype(dt), 0.3, 99)
    full = masked_distances(far, W)   # (only to pick prototypes; the comparison below is between device results)
    order = np.argsort(full[0])
    Wd = W.copy()
    Wd[order[1]] = Wd[order[0]]
    dist, idx = be.bmu_masked(Wd, 2, far)
    assert dist[0, 0] == dist[0, 1] and idx[0].tolist() == sorted([int(order[0]), int(order[1])])


# ---- 3. batch independence --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_results_do_not_depend_on_the_batch(be, dt):
    X, W, D = case(1000, 64, 129, 0.3, np.dtype(dt).name)
    X = X[:600]
    for k in (1, 2):
        dist, idx = be.bmu_masked(W, k, X)
        perm = np.random.default_rng(0).permutation(600)
        dp, ip = be.bmu_masked(W, k, X[perm])
        assert np.array_equal(ip, idx[perm]) and np.array_equal(dp, dist[perm])
        sub = np.sort(perm[:77])
        ds, is_ = be.bmu_masked(W, k, X[sub])
        assert np.array_equal(is_, idx[sub]) and np.array_equal(ds, dist[sub])
        old = be.masked_chunk_rows
        try:
            be.masked_chunk_rows = 256        # 600 rows: chunks of 256, 256 and 88
            dc, ic, filled = be.bmu_masked(W, k, X, want_filled=True)
        finally:
            be.masked_chunk_rows = old
        assert np.array_equal(ic, idx) and np.array_equal(dc, dist)
        assert np.array_equal(filled, fill_numpy(X, W, idx))


# ---- 4 - 6. estimators ----------------------------------------------------------------------------------------------
def _holes_in_every_row(X, frac, seed):
    Xn = punch(X, frac, seed)
    rng = np.random.default_rng(seed + 1)
    full = np.flatnonzero(~np.isnan(Xn).any(axis=1))
    keep = np.array([np.flatnonzero(~np.isnan(r))[0] for r in Xn[full]], dtype=np.int64)
    col = (keep + 1 + rng.integers(0, X.shape[1] - 1, full.size)) % X.shape[1]
    Xn[full, col] = np.nan
    assert np.isnan(Xn).any(axis=1).all() and not np.isnan(Xn).all(axis=1).any()
    return Xn


@pytest.fixture(scope="module")
def vq():
    from dbgsom_amd import SomVQ

    X, _ = gi.blobs_f32(5000, 24, 2)
    est = SomVQ(missing_values="nan", random_state=0, n_iter=20).fit(X)
    plain = SomVQ(random_state=0, n_iter=20).fit(X)
    assert np.array_equal(est.weights_, plain.weights_)       # the parameter changes nothing about fit
    return est, plain, X


def test_complete_rows_are_todays(vq):
    est, plain, X = vq
    Xn = punch(X[:3000], 0.2, 11)
    Xn[::2] = X[:3000:2]
    complete = ~np.isnan(Xn).any(axis=1)
    assert 1500 <= complete.sum() < 3000
    calls = []
    engine = est._engine()
    inner = engine.bmu_masked
    engine.bmu_masked = lambda *a, **kw: (calls.append(len(a[2])), inner(*a, **kw))[1]
    try:
        labels = est.predict(Xn)
        dist, idx = est._get_winning_neurons(Xn, 1)
        assert calls == [int((~complete).sum())] * 2
        assert np.array_equal(labels[complete], plain.predict(Xn[complete]))
        want = plain._get_winning_neurons(Xn[complete], 1)
        assert np.array_equal(dist[complete], want[0]) and np.array_equal(idx[complete], want[1])
        d2, i2 = est._get_winning_neurons(Xn, 2)
        want = plain._get_winning_neurons(Xn[complete], 2)
        assert np.array_equal(d2[complete], want[0]) and np.array_equal(i2[complete], want[1])
        del calls[:]
        assert np.array_equal(est.predict(X[:3000]), plain.predict(X[:3000]))
        assert est.calculate_quantization_error(X[:3000]) == plain.calculate_quantization_error(X[:3000])
        assert calls == []                                 # no NaN in the batch: no masked call at all
    finally:
        del engine.bmu_masked


@pytest.mark.parametrize("dt", DTYPES)
def test_impute(vq, dt):
    est, _, X = vq
    Xn = punch(X[:2000], 0.3, 12).astype(dt)
    Xn[::5] = X[:2000:5].astype(dt)
    before = Xn.copy()
    out = est.impute(Xn)
    holes = np.isnan(Xn)
    assert out.dtype == dt and out is not Xn and np.array_equal(Xn, before, equal_nan=True)
    assert not np.isnan(out).any() and np.array_equal(out[~holes], Xn[~holes])
    W = est.weights_.astype(np.float64)
    rows = holes.any(axis=1)
    D = masked_distances(Xn[rows], W)
    assert smallest_gap(D) > GAP
    idx = np.zeros(len(Xn), dtype=np.int64)
    idx[rows] = winners_of(D, 1)[1]
    assert np.array_equal(out[holes], W[idx][holes].astype(dt))
    # the fused device fill is the NumPy fill
    dist, got_idx, filled = est._engine().bmu_masked(W, 1, Xn[rows], want_filled=True)
    assert np.array_equal(got_idx, idx[rows]) and np.array_equal(filled, fill_numpy(Xn[rows], W, got_idx))
    assert np.array_equal(out[rows], filled)


def test_estimator_queries(vq):
    from dbgsom_amd import SomVQ

    est, plain, X = vq
    Xn = _holes_in_every_row(X[:2500], 0.3, 13)
    D = masked_distances(Xn, est.weights_)
    assert smallest_gap(D) > GAP
    want_dist, want_idx = winners_of(D, 1)
    assert np.array_equal(est.predict(Xn), want_idx)
    qe, want_qe = est.calculate_quantization_error(Xn), float(np.mean(want_dist))
    print(f"quantization error {qe!r}, oracle {want_qe!r}")
    assert abs(qe - want_qe) <= RTOL * want_qe
    with pytest.raises(ValueError, match="NaN"):
        SomVQ(missing_values="nan", random_state=0, n_iter=5).fit(np.vstack([Xn[:100], X[100:1000]]))
    with pytest.raises(ValueError, match="NaN"):
        SomVQ(random_state=0, n_iter=5).fit(np.vstack([Xn[:100], X[100:1000]]))
    with pytest.raises(ValueError, match="NaN"):
        plain.predict(Xn)                                   # the default estimator refuses as today
    with pytest.raises(ValueError, match="missing_values='nan'"):
        plain.impute(Xn)
    bad = Xn.copy()
    bad[1234] = np.nan
    for call in (est.predict, est.calculate_quantization_error, est.impute):
        with pytest.raises(ValueError, match="row 1234 .*no observed"):
            call(bad)
    with pytest.raises(ValueError, match="no observed"):   # the context call refuses such a row by itself too
        est._engine().bmu_masked(est.weights_, 1, bad[1230:1240])
    bad = Xn.copy()
    bad[7, 3] = np.inf
    with pytest.raises(ValueError, match="inf"):
        est.predict(bad)
    stored = sp.csr_matrix(np.where(np.isnan(Xn[:50]), 0, Xn[:50]).astype(np.float64))
    stored.data[5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        est.predict(stored)
    with pytest.raises(ValueError, match="NaN"):
        est.topographic_function(Xn)
    import copy

    bogus = copy.copy(est)
    bogus.missing_values = "bogus"
    with pytest.raises(ValueError, match="missing_values"):
        bogus.predict(Xn)


# ---- 7. classifier ----------------------------------------------------------------------------------------------------
def test_classifier_codes_the_imputed_rows():
    from dbgsom_amd import SomClassifier

    X, lab = gi.blobs_f32(5000, 24, 2)
    y = lab % 4
    clf = SomClassifier(missing_values="nan", random_state=0, n_iter=20).fit(X, y)
    Xn = punch(X[:400], 0.3, 14)
    Xn[::4] = X[:400:4]
    filled = clf.impute(Xn)
    assert np.array_equal(clf.predict_proba(Xn), clf.predict_proba(filled), equal_nan=True)
    assert np.array_equal(clf.predict(Xn), clf.predict(filled))
    assert np.array_equal(clf.transform(Xn), clf.transform(filled))
    clf.vertical_growth = True                              # (the branch is taken on the flag alone)
    with pytest.raises(ValueError, match="vertical_growth"):
        clf.predict_proba(Xn)
