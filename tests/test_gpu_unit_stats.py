"""MI355X: per-unit sums of a per-row quantity -- the raw calls of csrc/unit_sums.hip against the literal restatement of
tests/unit_stats.py bit for bit (outputs pre-filled with 0xFF bytes between guards, NaN in the padding of Z), the
targets of a context, and the estimators on HipBackend (unit_means, SomRegressor).  No test asserts on a clock."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from tests import device_abi as da
from tests import unit_stats as us

pytestmark = pytest.mark.gpu

GUARD = 8          # untouched elements in front of and behind every result
ESTATE = -4


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


@pytest.fixture(scope="module")
def be():
    from dbgsom_amd.backend import HipBackend

    b = HipBackend(0)
    yield b
    b.release()


def _sync():
    import torch

    torch.cuda.synchronize()


def _ptr(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _padded(A, ld):
    host = np.full((A.shape[0], ld), np.nan)
    host[:, :A.shape[1]] = A
    return da.dev(host)


class _Guarded:
    """rows x ld float64 filled with 0xFF bytes (every value reads NaN) with GUARD elements on either side"""

    def __init__(self, rows, cols, ld):
        import torch

        self.rows, self.cols, self.ld = rows, cols, ld
        self.t = torch.full((8 * (rows * ld + 2 * GUARD),), 0xFF, dtype=torch.uint8, device="cuda")
        self.ptr = ctypes.c_void_p(self.t.data_ptr() + 8 * GUARD)

    def read(self):
        a = self.t.cpu().numpy().view(np.uint64)
        ff = np.uint64(0xFFFFFFFFFFFFFFFF)
        n = self.rows * self.ld
        assert (a[:GUARD] == ff).all() and (a[GUARD + n:] == ff).all(), "a write outside the result"
        body = a[GUARD:GUARD + n].reshape(self.rows, self.ld)
        assert (body[:, self.cols:] == ff).all(), "a write behind a row of the result"
        return body[:, :self.cols].view(np.float64).copy()


def _fold_device(nat, be, units, Z, w, M, pad=0):
    """dbgsom_ctx_unit_sums_device with ldz = lds = V + pad -> (mass, sums)"""
    N, V = Z.shape
    ud, zd = da.dev(np.asarray(units, dtype=np.int64)), _padded(Z, V + pad)
    wd = None if w is None else da.dev(np.asarray(w, dtype=np.float64))
    mass, sums = _Guarded(M, 1, 1), _Guarded(M, V, V + pad)
    _sync()
    nat.call("dbgsom_ctx_unit_sums_device", be._ctx, _ptr(ud), _ptr(zd), V + pad, _ptr(wd), N, M, V, mass.ptr, sums.ptr,
             V + pad)
    return mass.read()[:, 0], sums.read()


# ---- 1. the fold, raw ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", us.N_LIST)
def test_fold_equals_the_restatement_over_the_table(nat, be, N):
    for M, V, pad, assign, weight in us.cases_for(N):
        units, Z, w, mass_ref, sums_ref = us.problem(N, M, V, assign, weight)
        mass, sums = _fold_device(nat, be, units, Z, w, len(mass_ref), pad)
        what = f"N={N} M={len(mass_ref)} V={V} pad={pad} {assign} {weight}"
        assert us.same_bits(mass, mass_ref), "mass: " + what
        assert us.same_bits(sums, sums_ref), "sums: " + what


@pytest.mark.parametrize("M,V,pad", us.SHAPES, ids=["M%d-V%d-pad%d" % s for s in us.SHAPES])
def test_fold_every_pairing_of_units_values_and_padding(nat, be, M, V, pad):
    units, Z, w, mass_ref, sums_ref = us.problem(1025, M, V, "mixed", "zeros")
    mass, sums = _fold_device(nat, be, units, Z, w, M, pad)
    assert us.same_bits(mass, mass_ref) and us.same_bits(sums, sums_ref)


def test_the_order_is_the_stated_one(nat, be):
    z = us.three_orders()
    _, sums = _fold_device(nat, be, np.zeros(len(z), dtype=np.int64), z[:, None], None, 1)
    assert sums[0, 0] == us.chain(z[:, None])[0] and sums[0, 0] != us.chain(z[::-1, None])[0] and sums[0, 0] != np.sum(z)
    z = us.blocked_list()
    units = np.zeros(len(z), dtype=np.int64)
    mass, sums = _fold_device(nat, be, units, z[:, None], None, 1)
    assert sums[0, 0] == us.fold(units, z, None, 1)[1][0, 0] == 2.0 ** 53 + 2.0
    assert sums[0, 0] != us.fold(units, z, None, 1, block=None)[1][0, 0] and mass[0] == 130.0
    _, sums = _fold_device(nat, be, units, z[:, None], np.ones(len(z)), 1)      # all-ones weights: the same bits
    assert sums[0, 0] == 2.0 ** 53 + 2.0


def test_a_nan_stays_in_its_unit_and_column(nat, be):
    units, Z, w, mass_ref, sums_ref = us.problem(1025, 64, 5, "random", "fractions")
    Zn = Z.copy()
    Zn[700, 2] = np.nan
    Zn[701, 4] = np.inf
    mass, sums = _fold_device(nat, be, units, Zn, w, 64, 3)
    hit = np.zeros(sums.shape, dtype=bool)
    hit[units[700], 2] = hit[units[701], 4] = True
    assert np.isnan(sums[units[700], 2]) and not np.isfinite(sums[units[701], 4])
    assert np.array_equal(us.bits(sums)[~hit], us.bits(sums_ref)[~hit]) and us.same_bits(mass, mass_ref)


def test_host_call_equals_device_call_and_counts_its_traffic(nat, be):
    units, Z, w, mass_ref, sums_ref = us.problem(1025, 65, 5, "mixed", "zeros")
    N, V, M = 1025, 5, 65
    for ww in (w, None):
        before = be.sample_traffic()
        mass, sums = np.full(M, np.nan), np.full((M, V), np.nan)
        u, z = np.ascontiguousarray(units), np.ascontiguousarray(Z)
        nat.call("dbgsom_ctx_unit_sums", be._ctx, u.ctypes.data, z.ctypes.data, None if ww is None else ww.ctypes.data, N, M,
                 V, mass.ctypes.data, sums.ctypes.data)
        after = be.sample_traffic()
        dm, dsum = _fold_device(nat, be, units, Z, ww, M)
        assert us.same_bits(mass, dm) and us.same_bits(sums, dsum)
        assert after["x_upload_bytes"] - before["x_upload_bytes"] == N * 8 * (1 + V + (ww is not None))
        assert after["x_download_bytes"] - before["x_download_bytes"] == M * (V + 1) * 8
        assert be.sample_traffic() == after                                    # the device call moves nothing
    assert us.same_bits(dm, us.fold(units, Z, None, M)[0])


@pytest.mark.parametrize("V", [1, 16])
@pytest.mark.parametrize("mode", [us.SQUARES, us.NORM])
def test_deviations(nat, be, mode, V):
    N, M = 257, 65
    rng = np.random.default_rng(V + mode)
    units = us.assignment("mixed", N, M, rng)
    Y, C = rng.normal(size=(N, V)) * 10.0 ** rng.integers(-3, 4, (N, 1)), rng.normal(size=(M, V))
    C[3] = np.nan
    ref = us.deviations(units, Y, C, mode)
    out = _Guarded(N, V if mode == us.SQUARES else 1, V + 2 if mode == us.SQUARES else 1)
    ud, yd, cd = da.dev(units), _padded(Y, V + 3), _padded(C, V + 1)
    _sync()
    nat.call("dbgsom_ctx_unit_deviations_device", be._ctx, _ptr(ud), _ptr(yd), V + 3, N, _ptr(cd), V + 1, M, V, mode, out.ptr,
             V + 2)
    got = out.read()
    assert us.same_bits(got if mode == us.SQUARES else got[:, 0], ref)
    assert (ref[(units < 0) | (units >= M)] == 0).all() and np.isnan(ref[units == 3]).all()


# ---- 2. targets of a context ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(11)
    centres = rng.normal(size=(6, 16)) * 4
    X = (centres[rng.integers(0, 6, 600)] + rng.normal(size=(600, 16))).astype(np.float64)
    Y = np.c_[X[:, 0] * 2 + rng.normal(size=600), np.sin(X[:, 1]), rng.normal(size=600) * 1e3]
    return X, Y


def test_target_statistics_follow_the_last_epoch(rows):
    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    X, Y = rows
    b = HipBackend(0)
    try:
        b.load(X)
        W = X[:9].copy()
        hop = np.abs(np.arange(9)[:, None] - np.arange(9)[None, :]).astype(np.float64)
        b.set_targets(Y)
        with pytest.raises(_native.DbgsomNativeError) as e:                     # no epoch yet: no winners in HBM
            b.target_statistics(None, 9, want_err=True)
        assert e.value.code == ESTATE
        res = b.epoch(W, hop, 1.0, 0.01, want_assignments=True)
        for w in (None, np.random.default_rng(3).integers(0, 3, 600).astype(np.float64)):
            b.set_sample_weight(w)
            got = b.target_statistics(None, 9, want_std=True, want_err=True)
            ref = us.statistics(res.winners, Y, w, 9)
            for g, r, name in zip(got, ref, ("mass", "mean", "std", "err")):
                assert us.same_bits(g, r), name
            given = b.target_statistics(res.winners, 9, want_std=True, want_err=True)   # winners handed over
            assert all(us.same_bits(g, r) for g, r in zip(given, ref))
        b.set_sample_weight(None)
        b.set_targets(None)                                                     # a detach
        with pytest.raises(RuntimeError):
            b.target_statistics(None, 9)
        rc = b._lib.dbgsom_ctx_target_statistics(b._ctx, None, 9, np.empty(9).ctypes.data, np.empty((9, 3)).ctypes.data,
                                                 None, None)
        assert rc == ESTATE
        b.set_targets(Y)
        b.load(X)                                                               # a reload detaches, and drops the winners
        assert b._targets is None
        rc = b._lib.dbgsom_ctx_target_statistics(b._ctx, None, 9, np.empty(9).ctypes.data, np.empty((9, 3)).ctypes.data,
                                                 None, None)
        assert rc == ESTATE
        b.set_targets(Y)
        with pytest.raises(_native.DbgsomNativeError) as e:
            b.target_statistics(None, 9)
        assert e.value.code == ESTATE
    finally:
        b.release()


# ---- 3. the estimators on HipBackend --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(rows):
    from dbgsom_amd import SomVQ

    X, _ = rows
    return SomVQ(n_iter=15, random_state=0, max_neurons=30).fit(X)


def test_unit_means_host_tensor_and_csr_give_the_same_bits(rows, fitted):
    import torch

    X, Y = rows
    w = np.random.default_rng(5).random(600)
    w[::7] = 0.0
    units = fitted.predict(X)
    M = len(fitted.weights_)
    for ww in (None, w):
        ref = us.statistics(units, Y, ww, M, want_err=False)
        host = fitted.unit_means(X, Y, sample_weight=ww, return_std=True, return_mass=True)
        csr = fitted.unit_means(sp.csr_matrix(X), Y, sample_weight=ww, return_std=True, return_mass=True)
        Xd = torch.from_numpy(X).cuda()
        dev = fitted.unit_means(Xd, torch.from_numpy(Y).cuda(), sample_weight=ww, return_std=True, return_mass=True)
        assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in dev)
        for k, name in enumerate(("mean", "std", "mass")):
            r = ref[(1, 2, 0)[k]]
            assert us.same_bits(host[k], r), name
            assert us.same_bits(csr[k], r), name + " (CSR)"
            assert us.same_bits(dev[k].cpu().numpy(), r), name + " (tensor)"
    flat = fitted.unit_means(X, Y[:, 0])
    assert flat.shape == (M,) and us.same_bits(flat, us.statistics(units, Y[:, :1], None, M)[1][:, 0])
    fitted.fit_mixture(X)
    q = fitted.posterior_mean(X[:50], fitted.unit_means(Xd, torch.from_numpy(Y).cuda()))    # as written, from a tensor
    assert q.shape == (50, 3) and us.same_bits(q, fitted.posterior_mean(X[:50], fitted.unit_means(X, Y)))


@pytest.fixture(scope="module")
def regressor(rows):
    from dbgsom_amd import SomRegressor

    X, Y = rows
    return SomRegressor(n_iter=15, random_state=0, max_neurons=30).fit(X, Y[:, :2])


def test_regressor_fit_from_host_and_tensor(rows, regressor):
    import torch

    from dbgsom_amd import SomRegressor

    X, Y = rows
    dev = SomRegressor(n_iter=15, random_state=0, max_neurons=30).fit(torch.from_numpy(X).cuda(),
                                                                      torch.from_numpy(Y[:, :2]).cuda())
    assert isinstance(dev.unit_targets_, np.ndarray) and us.same_bits(dev.unit_targets_, regressor.unit_targets_)
    assert us.same_bits(dev.unit_target_std_, regressor.unit_target_std_)
    units = regressor._get_winning_neurons(X, 1)[1]
    mass, mean, std, _ = us.statistics(units, Y[:, :2], None, len(regressor.weights_), want_err=False)
    assert us.same_bits(regressor.unit_targets_, mean) and us.same_bits(regressor.unit_target_std_, std)
    assert us.same_bits(regressor.unit_mass_, mass) and mass.sum() == 600 and regressor.n_outputs_ == 2


def test_regressor_prediction_modes(rows, regressor):
    import torch

    X, _ = rows
    Xd = torch.from_numpy(X).cuda()
    units = regressor._get_winning_neurons(X, 1)[1]
    p, s = regressor.predict(X, return_std=True)
    assert us.same_bits(p, regressor.unit_targets_[units]) and us.same_bits(s, regressor.unit_target_std_[units])
    pd_ = regressor.predict(Xd)
    assert isinstance(pd_, torch.Tensor) and pd_.is_cuda and us.same_bits(pd_.cpu().numpy(), p)
    try:
        regressor.set_params(prediction="knn", n_neighbors=1)
        assert us.same_bits(regressor.predict(X), p)
        regressor.set_params(n_neighbors=4)
        k = regressor.predict(X)
        assert k.shape == p.shape and np.isfinite(k).all()
        assert us.same_bits(regressor.predict(Xd).cpu().numpy(), k)              # elementwise only: the same bits
        exact = regressor.predict(regressor.weights_[:3])                        # distance 0: that unit's value
        assert us.same_bits(exact, regressor.unit_targets_[:3])
        with pytest.raises(ValueError, match="return_std"):
            regressor.predict(X, return_std=True)
        regressor.set_params(prediction="soft")
        with pytest.raises(ValueError, match="fit_mixture"):
            regressor.predict(X)
        regressor.fit_mixture(X)
        assert us.same_bits(regressor.predict(X), regressor.posterior_mean(X, regressor.unit_targets_))
        assert regressor.score(Xd, rows[1][:, :2]) == regressor.score(X, rows[1][:, :2])
    finally:
        regressor.set_params(prediction="bmu", n_neighbors=5)


def test_target_error_fit_keeps_the_prototypes_resident(rows):
    from dbgsom_amd import SomRegressor

    X, Y = rows
    est = SomRegressor(n_iter=24, random_state=0, max_neurons=40, growth_criterion="target_error").fit(X, Y[:, 0])
    tr, growth = est._training_traffic, est._growth_epochs
    assert len(est.weights_) >= 4 and np.isfinite(est.unit_targets_).all()
    assert tr["w_upload_calls"] == 1 and tr["w_download_calls"] == len(growth) + 2
    ref = 150 * -np.log(0.5) * np.linalg.norm(np.std(Y[:, :1], axis=0, ddof=1))
    assert est.growing_threshold_ == pytest.approx(ref, rel=1e-12)
    units = est._get_winning_neurons(X, 1)[1]
    assert us.same_bits(est.predict(X), est.unit_targets_[units])
