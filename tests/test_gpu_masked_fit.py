"""MI355X: fit on rows with missing entries (csrc/masked_fit.hip, the masked smoothing of csrc/smooth.hip, the masked
context calls) against the NumPy restatement of tests/masked_fit.py -- the sums within (n + 2) u sum |terms| of
np.longdouble sums with the counts exact, new prototypes to the tolerances of tests/test_gpu_parity.py, winners exactly
(the inputs meet the gap condition of tests/test_missing_cpu.py) -- and the estimators under
``missing_values="nan-fit"``."""
import numpy as np
import pytest

from tests import device_abi as da
from tests import golden_inputs as gi
from tests import masked_fit as mf
from tests.test_missing_cpu import DTYPES, GAP, RTOL, case, masked_bmu, masked_distances, punch

pytestmark = pytest.mark.gpu

NAME = {"float32": "f32", "float64": "f64"}


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


def _sync():
    import torch

    torch.cuda.synchronize()


def _full(shape, value, dtype):
    import torch

    return torch.full(shape, value, dtype=getattr(torch, dtype), device="cuda")


def _stage_junk(A, ld, offset_elems):
    """da.stage's layout with finite junk instead of NaN around the rows"""
    import torch

    buf = da.host_rows(A, ld, offset_elems)
    body = buf[offset_elems:].reshape(A.shape[0], ld)
    body[:, A.shape[1]:] = 3.0e30
    buf[:offset_elems] = -7.0
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + offset_elems * A.dtype.itemsize


def _split(v, M, d):
    Md = M * d
    return v[:Md].reshape(M, d), v[Md:2 * Md].reshape(M, d), v[2 * Md:3 * Md].reshape(M, d), v[3 * Md:3 * Md + M], v[3 * Md + M:]


def _accumulate_masked(nat, X, ldx, off_bytes, winners, kw, dist, M, junk=False):
    """dbgsom_accumulate_masked on torch tensors, twice (the same bits) -> ((S, K, A, a, E), status)"""
    lib = nat.load()
    N, d = X.shape
    dtype = NAME[X.dtype.name]
    off = off_bytes // X.dtype.itemsize
    xt, xptr = _stage_junk(X, ldx, off) if junk else da.stage(X, ldx, off, dtype)
    win_t, kw_t, dist_t = da.dev(winners.copy()), da.dev(kw.copy()), da.dev(dist.copy())
    nbytes = lib.dbgsom_accumulate_masked_workspace_bytes(N, d, M)
    assert nbytes > 0
    ws_t, ws = da.workspace(nbytes)
    outs = []
    for _ in range(2):
        sums = _full((M * (3 * d + 2),), float("nan"), "float64")
        st = _full((1,), 77, "int32")
        nat.call("dbgsom_accumulate_masked", xptr, da.CODE[dtype], N, d, ldx, win_t.data_ptr(), kw_t.data_ptr(),
                 dist_t.data_ptr(), M, sums.data_ptr(), st.data_ptr(), ws, nbytes, da.stream())
        _sync()
        outs.append((sums.cpu().numpy(), int(st.cpu()[0])))
    assert np.array_equal(outs[0][0], outs[1][0], equal_nan=True) and outs[0][1] == outs[1][1]
    return _split(outs[0][0], M, d), outs[0][1]


# ---- 1. dbgsom_accumulate_masked ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("frac", mf.ACC_FRACS)
@pytest.mark.parametrize("N,d,M,ldx,off_bytes", mf.ACC_SHAPES)
def test_accumulate_masked_against_longdouble_sums(nat, N, d, M, ldx, off_bytes, frac, dt):
    name = np.dtype(dt).name
    c = mf.accumulate_case(N, d, M, frac, name)
    X, win, kw, dist = c["X"], c["winners"], c["kw"], c["dist"]
    (S, K, A, a, E), st = _accumulate_masked(nat, X, ldx, off_bytes, win, kw, dist, M)
    (Sr, Kr, Ar, ar, Er), (TS, TK, TE) = mf.accumulate_reference(N, d, M, frac, name)
    assert st == 0
    for part in (S, K, A, a, E):
        assert not np.isnan(part).any()
    assert np.array_equal(A, Ar) and np.array_equal(a, ar) and a.sum() == N          # exact, no row left out
    for label, got, ref, T, n in (("S", S, Sr, TS, A), ("K", K, Kr, TK, A), ("E", E, Er, TE, a)):
        n_ = np.asarray(n, dtype=np.longdouble)
        bound = (n_ + 2) * da.U * T + n_ * da.UL * T                                 # device_abi.sums_within_bound, n per entry
        err = np.abs(np.asarray(got, dtype=np.longdouble) - ref)
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
        print(f"{label}: largest error / bound {worst:.3f}")
        assert np.all(err <= bound), label
    unseen = A == 0
    assert (S[unseen] == 0).all() and (K[unseen] == 0).all()
    if c["big"] is not None:
        assert a[c["big"]] > 128 and a[c["empty"]] == 0
        assert (S[c["empty"]] == 0).all() and (K[c["empty"]] == 0).all() and (A[c["empty"]] == 0).all() and E[c["empty"]] == 0
        j, col = c["blind"]
        assert a[j] > 0 and S[j, col] == 0 and K[j, col] == 0 and A[j, col] == 0
    # NaN (above) or finite junk in the padding columns and in front of the rows: the same bits
    if ldx > d or off_bytes:
        other, _ = _accumulate_masked(nat, X, ldx, off_bytes, win, kw, dist, M, junk=True)
        assert all(np.array_equal(g, w) for g, w in zip((S, K, A, a, E), other))


@pytest.mark.parametrize("dt", DTYPES)
def test_accumulate_masked_status_and_skipped_rows(nat, dt):
    N, d, M, ldx, off_bytes = mf.ACC_SHAPES[1]
    c = mf.accumulate_case(N, d, M, 0.3, np.dtype(dt).name)
    win = c["winners"].copy()
    win[[3, 100, 256]] = [-1, M, 1 << 40]
    (S, K, A, a, E), st = _accumulate_masked(nat, c["X"], ldx, off_bytes, win, c["kw"], c["dist"], M)
    assert st != 0 and a.sum() == N - 3
    Sr, Kr, Ar, ar, Er = mf.masked_sums(c["X"], win, c["kw"], c["dist"], M)
    assert np.array_equal(A, Ar) and np.array_equal(a, ar)
    np.testing.assert_allclose(S, Sr, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(E, Er, rtol=1e-12)


# ---- 2. dbgsom_smooth_masked --------------------------------------------------------------------------------------
def _smooth_masked(nat, S, K, A, a, E, hop, sigma, W_old):
    lib = nat.load()
    M, d = S.shape
    sums = da.dev(np.concatenate([S.reshape(-1), K.reshape(-1), A.reshape(-1), a, E]))
    hop_t, wo = da.dev(hop.astype(np.float32)), da.dev(W_old)
    wn, chg = _full((M, d), float("nan"), "float64"), _full((1,), float("nan"), "float64")
    nbytes = lib.dbgsom_smooth_masked_workspace_bytes(M, d)
    ws_t, ws = da.workspace(nbytes)
    nat.call("dbgsom_smooth_masked", sums.data_ptr(), M, d, hop_t.data_ptr(), sigma, wo.data_ptr(), wn.data_ptr(),
             chg.data_ptr(), ws, nbytes, da.stream())
    _sync()
    return wn.cpu().numpy(), float(chg.cpu()[0])


@pytest.mark.parametrize("d", mf.SMOOTH_D)
@pytest.mark.parametrize("M", mf.SMOOTH_M)
def test_smooth_masked_against_the_oracle(nat, M, d):
    from oracle import som_oracle as o

    S, K, A, a, E, hop, W_old, sigma = mf.smooth_case(M, d)
    assert (A == 0).any() or M * d < 8
    Wn, chg = _smooth_masked(nat, S, K, A, a, E, hop, sigma, W_old)
    want = mf.masked_smooth(S, K, A, hop, sigma, W_old)
    np.testing.assert_allclose(Wn, want, rtol=mf.W_RTOL, atol=mf.W_ATOL)
    assert chg == pytest.approx(o.change_total(W_old, want), rel=1e-10)


@pytest.mark.parametrize("M,d", [(4, 3), (37, 17), (300, 130)])
def test_smooth_masked_keeps_what_nobody_in_reach_observed(nat, M, d):
    S, K, A, a, E, hop, W_old, sigma = mf.smooth_case(M, d, split=True)
    Wn, _ = _smooth_masked(nat, S, K, A, a, E, hop, sigma, W_old)
    half = M // 2
    assert np.array_equal(Wn[half:, 0], W_old[half:, 0])                             # bitwise
    assert not np.array_equal(Wn[:half, 0], W_old[:half, 0])
    np.testing.assert_allclose(Wn, mf.masked_smooth(S, K, A, hop, sigma, W_old), rtol=mf.W_RTOL, atol=mf.W_ATOL)


# ---- 3. the context: load(X, incomplete=True), epoch_masked, the resident bmu --------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,d,M", mf.EPOCH_SHAPES)
def test_epoch_masked_against_the_oracle(N, d, M, dt):
    from dbgsom_amd.backend import HipBackend

    X, W, D = case(N, d, M, 0.3, np.dtype(dt).name)
    rows = max(1, int(np.sqrt(M)))
    while M % rows:
        rows -= 1
    hop = gi.lattice_hops(rows, M // rows).astype(np.float64)
    sigma, gamma = 1.5, float(np.nanvar(X, axis=0).sum() ** -1)
    be = HipBackend(0).load(X, incomplete=True)
    try:
        res = be.epoch_masked(W, hop, sigma, gamma, want_assignments=True)
        want_dist, want_idx = masked_bmu(X, W, 1)
        assert np.array_equal(res.winners, want_idx)                                  # every row
        np.testing.assert_allclose(res.distances, want_dist, rtol=RTOL, atol=0)
        ref = mf.masked_epoch(X, W, hop, sigma, gamma, winners=res.winners, distances=res.distances)
        np.testing.assert_allclose(res.new_weights, ref.new_weights, rtol=mf.W_RTOL, atol=mf.W_ATOL)
        np.testing.assert_allclose(res.errors, ref.errors, rtol=1e-12)
        assert np.array_equal(res.activations, ref.activations)
        assert res.change_total == pytest.approx(ref.change_total, rel=1e-9)
        d2, i2 = be.bmu(W, 2)
        q2, j2 = be.bmu_masked(W, 2, X)
        assert np.array_equal(i2, j2) and np.array_equal(d2, q2)
        assert be.quantization_error(W) == pytest.approx(float(np.mean(want_dist)), rel=RTOL)
        for call in (lambda: be.epoch(W, hop, sigma, gamma), lambda: be.partition(W), lambda: be.column_moments(),
                     lambda: be.update(W, hop, sigma, np.ones(N), res.winners, res.distances)):
            with pytest.raises(ValueError, match="missing entries"):
                call()
    finally:
        be.release()
    be.load(np.where(np.isnan(X), 0, X))                                               # the next load is complete again
    assert be._get("incomplete") == 0
    be.bmu(W, 1)
    be.release()


def test_ordinary_bmu_refuses_incomplete_residents(nat):
    from dbgsom_amd.backend import HipBackend

    X, W, _ = case(257, 17, 5, 0.3, "float64")
    be = HipBackend(0).load(X, incomplete=True)
    try:
        idx, dist = np.empty(257, dtype=np.int64), np.empty(257)
        W64 = np.ascontiguousarray(W)
        rc = nat.load().dbgsom_ctx_bmu(be._ctx, W64.ctypes.data, 5, 1, 0, idx.ctypes.data, dist.ctypes.data)
        assert rc == -1 and b"missing entries" in nat.load().dbgsom_last_error()
        be.set_sample_weight(np.ones(257))
        with pytest.raises(ValueError, match="sample weights"):
            be.bmu(W, 1)
    finally:
        be.release()
    be.load(np.where(np.isnan(X), 0, X))
    with pytest.raises(ValueError, match="not marked incomplete"):
        nat.call("dbgsom_ctx_bmu_masked", be._ctx, W64.ctypes.data, 5, 1, idx.ctypes.data, dist.ctypes.data)
    be.release()


# ---- 4. the estimators ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from dbgsom_amd import SomVQ

    X, lab = gi.blobs_f32(3000, 24, 2)
    Xn = punch(X, 0.2, 13)
    est = SomVQ(missing_values="nan-fit", random_state=0, n_iter=20).fit(Xn)
    return est, X, Xn, lab


def test_estimator_on_rows_with_holes(fitted):
    est, X, Xn, _ = fitted
    assert np.isfinite(est.weights_).all()
    D = masked_distances(Xn, est.weights_)
    S = np.sort(D, axis=1)
    clear = (S[:, 1] - S[:, 0]) / S[:, 1] > GAP
    assert (~clear).sum() <= 3
    assert np.array_equal(est.labels_[clear], np.argmin(D, axis=1)[clear])
    assert est.quantization_error_ == pytest.approx(float(np.mean(S[:, 0])), rel=RTOL)
    filled = est.impute(Xn)
    got, base = mf.impute_rmse(X, Xn, filled), mf.mean_fill_rmse(X, Xn)
    print(f"RMSE over the punched cells: impute {got:.4f}, column means {base:.4f}")
    assert got < base


def test_estimator_on_complete_rows_is_the_default_fit(fitted):
    from dbgsom_amd import SomVQ

    _, X, _, _ = fitted
    a = SomVQ(missing_values="nan-fit", random_state=0, n_iter=12).fit(X[:1500])
    b = SomVQ(random_state=0, n_iter=12).fit(X[:1500])
    assert np.array_equal(a.weights_, b.weights_) and np.array_equal(a.labels_, b.labels_)


def test_classifier_and_refusals(fitted):
    from dbgsom_amd import SomClassifier, SomVQ

    _, X, Xn, lab = fitted
    y = lab[:1200] % 3
    clf = SomClassifier(missing_values="nan-fit", random_state=0, n_iter=12, max_neurons=30).fit(Xn[:1200], y)
    pred = clf.predict(punch(X[:100], 0.3, 5))
    assert pred.shape == (100,) and set(pred) <= set(np.unique(y))
    small = Xn[:400]
    bad = small.copy()
    bad[5, 1] = np.inf
    with pytest.raises(ValueError, match="inf"):
        SomVQ(missing_values="nan-fit", n_iter=3).fit(bad)
    bad = small.copy()
    bad[17] = np.nan
    with pytest.raises(ValueError, match="row 17 .*no observed"):
        SomVQ(missing_values="nan-fit", n_iter=3).fit(bad)
    bad = small.copy()
    bad[1:, 4] = np.nan
    with pytest.raises(ValueError, match="column 4 "):
        SomVQ(missing_values="nan-fit", n_iter=3).fit(bad)
    with pytest.raises(ValueError, match="sample_weight"):
        SomVQ(missing_values="nan-fit", n_iter=3).fit(small, sample_weight=np.ones(400))
    with pytest.raises(ValueError, match="vertical_growth"):
        SomVQ(missing_values="nan-fit", n_iter=3, vertical_growth=True).fit(small)
    with pytest.raises(ValueError, match="sharded_input"):
        SomVQ(missing_values="nan-fit", n_iter=3, sharded_input=True).fit(small)
    with pytest.raises(ValueError, match="NaN"):
        SomVQ(missing_values="nan", n_iter=3).fit(small)
