"""CPU: per-unit statistics -- the restatement of csrc/unit_sums.hip (tests/unit_stats.py, and the vectorised one
HotPathBackend runs) against np.longdouble and against lists whose order shows, the deviations against exact rational
arithmetic, ``unit_means`` / ``SomRegressor`` / ``growth_criterion="target_error"`` on a CPU stand-in backend, every
refusal, and the argument errors of the new entries of the C ABI (reported before any device work)."""
import math
import pickle
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.base import clone

from dbgsom_amd import SomClassifier, SomRegressor, SomVQ, _native
from dbgsom_amd import backend as bk
from dbgsom_amd.lattice import GrowingLattice
from tests import unit_stats as us

EINVAL = -1


# ---- the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [n for n in us.N_LIST if n])
def test_restatement_within_its_bound_of_longdouble(N):
    for M, V, _, assign, weight in us.cases_for(N):
        if weight == "zeros":
            continue                      # (NaN and infinities under weight 0 are never read: covered below)
        units, Z, w, mass, sums = us.problem(N, M, V, assign, weight)
        ref, lim = us.longdouble_bound(units, Z, w, len(mass))
        got = np.hstack([sums, mass[:, None]]).astype(np.longdouble)
        assert (np.abs(got - ref) <= lim).all(), (N, M, V, assign, weight)


@pytest.mark.parametrize("N", us.N_LIST)
def test_backend_restatement_equals_the_literal_one(N):
    for M, V, _, assign, weight in us.cases_for(N):
        units, Z, w, mass, sums = us.problem(N, M, V, assign, weight)
        m2, s2 = bk.unit_fold(units, Z, w, len(mass))
        assert us.same_bits(m2, mass) and us.same_bits(s2, sums), (N, M, V, assign, weight)


def test_the_order_has_teeth():
    z = us.three_orders()
    asc, desc, pair = us.chain(z[:, None])[0], us.chain(z[::-1, None])[0], np.sum(z)
    assert len({float(asc), float(desc), float(pair)}) == 3
    units = np.zeros(len(z), dtype=np.int64)
    assert bk.unit_fold(units, z[:, None], None, 1)[1][0, 0] == asc
    z = us.blocked_list()
    units = np.zeros(130, dtype=np.int64)
    flat, blocked = us.fold(units, z, None, 1, block=None)[1][0, 0], us.fold(units, z, None, 1)[1][0, 0]
    assert flat == 2.0 ** 53 and blocked == 2.0 ** 53 + 2.0
    assert bk.unit_fold(units, z[:, None], None, 1)[1][0, 0] == blocked


def test_ones_zero_weights_and_empty_units():
    units, Z, _, mass, sums = us.problem(1025, 65, 5, "mixed", "none")
    m1, s1 = bk.unit_fold(units, Z, np.ones(1025), 65)
    assert us.same_bits(m1, mass) and us.same_bits(s1, sums)               # all-ones weights: the bits of no weights
    units, Z, w, mass, sums = us.problem(1025, 65, 5, "random", "zeros")
    assert np.isnan(Z[w == 0]).any() and np.isinf(Z[w == 0]).any()
    assert np.isfinite(sums).all()                                           # weight 0 over NaN / inf is skipped
    keep = w != 0
    mk, sk = us.fold(units[keep], Z[keep], w[keep], 65)
    assert us.same_bits(mk, mass) and us.same_bits(sk, sums)
    units, Z, w, mass, sums = us.problem(130, 3, 2, "one", "fractions")
    for a in (mass[[0, 2]], sums[[0, 2]]):                                   # +0.0 bitwise for an empty unit
        assert (a.view(np.uint64) == 0).all()
    m0, s0 = bk.unit_fold(np.empty(0, np.int64), np.empty((0, 4)), None, 7)
    assert m0.shape == (7,) and s0.shape == (7, 4) and not m0.view(np.uint64).any() and not s0.view(np.uint64).any()


def test_a_nan_poisons_its_own_unit_and_column_only():
    units, Z, w, mass, sums = us.problem(257, 64, 5, "random", "fractions")
    Zn = Z.copy()
    Zn[100, 3] = np.nan
    m, s = bk.unit_fold(units, Zn, w, 64)
    hit = np.zeros(s.shape, dtype=bool)
    hit[units[100], 3] = True
    assert np.isnan(s[hit]).all() and np.array_equal(us.bits(s)[~hit], us.bits(sums)[~hit]) and us.same_bits(m, mass)


def _exact(x):
    return float(x)          # float(Fraction) rounds to nearest, ties to even


def test_deviations_hold_their_stated_roundings():
    rng = np.random.default_rng(2)
    N, M, V = 40, 5, 6
    units = us.assignment("mixed", N, M, rng)
    Y, C = rng.normal(size=(N, V)) * 10.0 ** rng.integers(-3, 4, (N, 1)), rng.normal(size=(M, V))
    for fn in (us.deviations, bk.unit_deviations):
        sq, nrm = fn(units, Y, C, us.SQUARES), fn(units, Y, C, us.NORM)
        for i in range(N):
            j = units[i]
            if not 0 <= j < M:
                assert not sq[i].view(np.uint64).any() and nrm[i] == 0.0 and not np.signbit(nrm[i])
                continue
            s = 0.0
            for v in range(V):
                d = _exact(Fraction(Y[i, v]) - Fraction(C[j, v]))            # the difference rounded
                q = _exact(Fraction(d) * Fraction(d))                        # the square rounded
                assert sq[i, v] == q
                s = _exact(Fraction(s) + Fraction(q))                        # the add rounded
            assert nrm[i] == math.sqrt(s)                                    # the root correctly rounded


def test_unit_statistics_default_is_the_restatement():
    units, Z, w, _, _ = us.problem(257, 64, 5, "mixed", "integers")
    got = bk.HotPathBackend().unit_statistics(units, Z, w, 64, want_std=True, want_err=True)
    for g, r in zip(got, us.statistics(units, Z, w, 64)):
        assert us.same_bits(g, r)
    mass, mean, std, err = got
    assert np.isnan(mean[mass == 0]).all() and (err[mass > 0] >= 0).all()
    assert bk.HotPathBackend().unit_statistics(units, Z, w, 64)[2:] == (None, None)


# ---- unit_means and SomRegressor on the stand-in --------------------------------------------------------------------
def _rows():
    rng = np.random.default_rng(11)
    centres = rng.normal(size=(6, 8)) * 4
    X = centres[rng.integers(0, 6, 400)] + rng.normal(size=(400, 8))
    Y = np.c_[X[:, 0] * 2 + rng.normal(size=400), np.sin(X[:, 1]), rng.normal(size=400) * 1e3]
    return X, Y


@pytest.fixture(scope="module")
def rows():
    return _rows()


@pytest.fixture(scope="module")
def vq(rows):
    return SomVQ(n_iter=12, random_state=0, max_neurons=20, backend=us.UnitStatsOracleBackend()).fit(rows[0])


def test_unit_means_on_the_stand_in(rows, vq):
    X, Y = rows
    M, units = len(vq.weights_), vq.predict(X)
    w = np.random.default_rng(5).random(400)
    w[::7] = 0.0
    for ww in (None, w):
        mass, mean, std, _ = us.statistics(units, Y, ww, M, want_err=False)
        got = vq.unit_means(X, Y, sample_weight=ww, return_std=True, return_mass=True)
        assert us.same_bits(got[0], mean) and us.same_bits(got[1], std) and us.same_bits(got[2], mass)
        csr = vq.unit_means(sp.csr_matrix(X), Y, sample_weight=ww, return_std=True, return_mass=True)
        assert all(us.same_bits(a, b) for a, b in zip(csr, got))
    flat = vq.unit_means(X, Y[:, 0])
    assert flat.shape == (M,) and us.same_bits(flat, mean_of(units, Y[:, :1], M))
    assert us.same_bits(vq.unit_means(X, Y[:, 0].astype(np.float32)), mean_of(units, Y[:, :1].astype(np.float32), M))
    only, mass = vq.unit_means(X, Y, return_mass=True)
    assert only.shape == (M, 3) and mass.sum() == 400
    vq.fit_mixture(X)
    q = vq.posterior_mean(X[:20], vq.unit_means(X, Y))                       # as written
    assert q.shape == (20, 3) and np.isfinite(q).all()


def mean_of(units, Z, M):
    return us.statistics(units, Z, None, M, want_std=False, want_err=False)[1][:, 0]


def test_unit_means_refusals(rows, vq):
    X, Y = rows
    for bad, word in ((Y[:-1], "rows"), (Y[:, :, None], "dimensions"), (np.zeros((400, 17)), "17 columns"),
                      (np.array(["a"] * 400), "dtype"), (Y.astype(complex), "dtype"), (np.zeros((400, 0)), "no column")):
        with pytest.raises(ValueError, match=word):
            vq.unit_means(X, bad)
    for bad in (np.ones(399), np.ones((400, 1)), -np.ones(400), np.r_[np.nan, np.ones(399)], np.r_[np.inf, np.ones(399)]):
        with pytest.raises(ValueError, match="sample_weight must be 400 finite numbers >= 0"):
            vq.unit_means(X, Y, sample_weight=bad)


@pytest.fixture(scope="module")
def reg(rows):
    X, Y = rows
    return SomRegressor(n_iter=12, random_state=0, max_neurons=20, backend=us.UnitStatsOracleBackend()).fit(X, Y[:, :2])


def test_regressor_attributes_and_prediction_modes(rows, reg):
    X, Y = rows
    M = len(reg.weights_)
    units = reg._get_winning_neurons(X, 1)[1]
    mass, mean, std, _ = us.statistics(units, Y[:, :2], None, M, want_err=False)
    assert us.same_bits(reg.unit_targets_, mean) and us.same_bits(reg.unit_target_std_, std)
    assert us.same_bits(reg.unit_mass_, mass) and reg.n_outputs_ == 2 and not hasattr(reg, "classes_")
    assert np.array_equal(units, SomVQ.predict(reg, X))
    p, s = reg.predict(X, return_std=True)
    assert us.same_bits(p, reg.unit_targets_[units]) and us.same_bits(s, reg.unit_target_std_[units])
    assert 0.0 < reg.score(X, Y[:, :2]) <= 1.0
    try:
        reg.set_params(prediction="knn", n_neighbors=1)
        assert us.same_bits(reg.predict(X), p)                               # one neighbour: "bmu"
        reg.set_params(n_neighbors=3)
        dist, idx = reg.kneighbors(X, 3)
        num, den = np.zeros((400, 2)), np.zeros(400)
        for t in range(3):
            num, den = num + (1.0 / dist[:, t])[:, None] * reg.unit_targets_[idx[:, t]], den + 1.0 / dist[:, t]
        assert np.array_equal(reg.predict(X), num / den[:, None])
        assert us.same_bits(reg.predict(reg.weights_[:2]), reg.unit_targets_[:2])      # distance 0: that unit's value
        reg.set_params(n_neighbors=1000)
        assert reg.predict(X).shape == (400, 2)                              # min(n_neighbors, M)
        with pytest.raises(ValueError, match="return_std needs prediction='bmu'"):
            reg.predict(X, return_std=True)
        reg.set_params(prediction="soft")
        with pytest.raises(ValueError, match="fit_mixture"):
            reg.predict(X)
        reg.fit_mixture(X)
        assert us.same_bits(reg.predict(X), reg.posterior_mean(X, reg.unit_targets_))
        reg.set_params(prediction="nearest")
        with pytest.raises(ValueError, match="SomRegressor: prediction must be one of"):
            reg.predict(X)
    finally:
        reg.set_params(prediction="bmu", n_neighbors=5)


def test_regressor_one_output_weights_csr_pickle_clone(rows):
    X, Y = rows
    w = np.random.default_rng(1).integers(0, 3, 400).astype(np.float64)
    kw = dict(n_iter=10, random_state=0, max_neurons=16)
    est = SomRegressor(backend=us.UnitStatsOracleBackend(), **kw).fit(X, Y[:, 0], sample_weight=w)
    M = len(est.weights_)
    assert est.unit_targets_.shape == est.unit_target_std_.shape == est.unit_mass_.shape == (M,) and est.n_outputs_ == 1
    units = est._get_winning_neurons(X, 1)[1]
    mass, mean, std, _ = us.statistics(units, Y[:, :1], w, M, want_err=False)
    assert us.same_bits(est.unit_targets_, mean[:, 0]) and us.same_bits(est.unit_mass_, mass) and mass.sum() == w.sum()
    assert est.predict(X).shape == (400,) and est.predict(X, return_std=True)[1].shape == (400,)
    csr = SomRegressor(backend=us.UnitStatsOracleBackend(), **kw).fit(sp.csr_matrix(X), Y[:, 0], sample_weight=w)
    assert len(csr.weights_) == M and np.allclose(csr.unit_targets_, est.unit_targets_, rtol=1e-9, equal_nan=True)
    assert us.same_bits(csr.predict(sp.csr_matrix(X)), csr.predict(X))
    back = pickle.loads(pickle.dumps(est))
    back.set_params(backend=us.UnitStatsOracleBackend())
    assert us.same_bits(back.predict(X), est.predict(X)) and "_fit_targets" not in est.__dict__
    params = clone(est).get_params()
    assert params["prediction"] == "bmu" and params["n_neighbors"] == 5 and params["growth_criterion"] == "quantization_error"
    assert set(SomVQ().get_params()) | {"prediction", "n_neighbors"} == set(params)
    lst = SomRegressor(backend=us.UnitStatsOracleBackend(), **kw).fit(X, list(Y[:, 0]), sample_weight=w)
    assert us.same_bits(lst.unit_targets_, est.unit_targets_)


def test_regressor_refusals(rows):
    X, Y = rows
    mk = lambda **kw: SomRegressor(n_iter=3, random_state=0, backend=us.UnitStatsOracleBackend(), **kw)   # noqa: E731
    for kw, word in ((dict(vertical_growth=True), "vertical_growth"), (dict(sharded_input=True), "one process"),
                     (dict(growth_criterion="entropy"), "growth_criterion"), (dict(prediction="mean"), "prediction"),
                     (dict(n_neighbors=0), "n_neighbors")):
        with pytest.raises(ValueError, match="SomRegressor.*" + word):
            mk(**kw).fit(X, Y[:, 0])
    for y, word in ((np.zeros((400, 17)), "17 columns"), (Y[:-1, 0], "shape"), (None, "requires y"),
                    (np.r_[np.nan, Y[1:, 0]], "NaN or an infinity"), (np.zeros((400, 2, 2)), "shape"),
                    (np.array(["a"] * 400), "real numbers")):
        with pytest.raises(ValueError, match="SomRegressor.*" + word):
            mk().fit(X, y)
    for est in (SomVQ, SomClassifier):
        with pytest.raises(ValueError, match="target_error"):
            est(n_iter=3, growth_criterion="target_error", backend=us.UnitStatsOracleBackend()).fit(X, (Y[:, 0] > 0).astype(int))


# ---- growth on the target's error ------------------------------------------------------------------------------------
def _two_clusters():
    """A: 300 rows spread wide in X, y = 0.  B: 300 rows packed tightly in X around (10, 0), y = 20 (x_0 - 10): the
    target varies inside B only, while nearly all of X's spread is A's."""
    rng = np.random.default_rng(3)
    A = rng.normal(size=(300, 2))
    B = np.array([10.0, 0.0]) + rng.normal(size=(300, 2)) * 0.3
    return np.r_[A, B], np.r_[np.zeros(300), 20 * (B[:, 0] - 10.0)]


def test_target_error_is_what_the_lattice_sees(monkeypatch):
    """The property: on the same map (same seed, same start rows, same first epoch) the unit that owns B carries the
    largest error under "target_error" and a unit of A the largest under "quantization_error" -- the two criteria
    point the first growth step at different units; and the errors handed over are the restatement's err_j."""
    X, y = _two_clusters()
    seen = {}
    real = GrowingLattice.set_errors

    def spy(self, errors):
        seen.setdefault(crit, []).append(np.array(errors))
        return real(self, errors)

    monkeypatch.setattr(GrowingLattice, "set_errors", spy)
    fits, start = {}, {}
    for crit in ("quantization_error", "target_error"):
        be = us.UnitStatsOracleBackend()
        fits[crit] = SomRegressor(n_iter=60, random_state=0, max_neurons=20, growth_criterion=crit, backend=be).fit(X, y)
        assert len(be.target_calls) == (len(seen[crit]) if crit == "target_error" else 0)
        start[crit] = be.epoch_weights[0]
    (Wq, eq), (Wt, et) = [(start[c], seen[c][0]) for c in ("quantization_error", "target_error")]
    assert np.array_equal(Wq, Wt) and len(eq) == len(et) == 4                # the same 2 x 2 start map
    in_b = np.linalg.norm(Wt - np.array([10.0, 0.0]), axis=1) < 2.0
    assert 1 <= in_b.sum() <= 3                                              # start rows from both clusters
    assert in_b[np.argmax(et)] and not in_b[np.argmax(eq)]
    units = us.UnitStatsOracleBackend().bmu(Wt, 1, X)[1]
    assert us.same_bits(et, us.statistics(units, y, None, 4)[3])             # err_j of the epoch's own winners
    # the threshold is the "se" formula on y, and at the end the map has spent more units on B
    for crit in fits:
        ref = X if crit == "quantization_error" else y[:, None]
        assert fits[crit].growing_threshold_ == pytest.approx(150 * -np.log(0.5) * np.linalg.norm(np.std(ref, axis=0, ddof=1)),
                                                               rel=1e-12)
    owners = {c: len(np.unique(f._get_winning_neurons(X[300:], 1)[1])) for c, f in fits.items()}
    assert owners["target_error"] > owners["quantization_error"]
    assert fits["target_error"].score(X, y) > fits["quantization_error"].score(X, y)


def test_target_threshold_classical_and_weighted():
    X, y = _two_clusters()
    Y = np.c_[y, -2 * y, y + 1]
    w = np.random.default_rng(0).integers(0, 4, 600).astype(np.float64)
    kw = dict(n_iter=4, random_state=0, growth_criterion="target_error")
    est = SomRegressor(threshold_method="classical", backend=us.UnitStatsOracleBackend(), **kw).fit(X, Y)
    assert est.growing_threshold_ == -3 * np.log(0.5)
    est = SomRegressor(backend=us.UnitStatsOracleBackend(), **kw).fit(X, Y, sample_weight=w)
    rep = np.repeat(Y, w.astype(int), axis=0)
    assert est.growing_threshold_ == pytest.approx(150 * -np.log(0.5) * np.linalg.norm(np.std(rep, axis=0, ddof=1)), rel=1e-10)
    assert est.unit_mass_.sum() == w.sum()


# ---- the hook keeps the other estimators as they were ---------------------------------------------------------------
def test_encode_targets_hook_keeps_vq_and_classifier():
    from sklearn.datasets import load_digits

    dg = load_digits()
    X, y = dg.data[:500], dg.target[:500] * 3 + 1

    class Before(SomClassifier):
        def _encode_targets(self, yy):                                       # the statement fit had inline
            classes, yy = np.unique(yy, return_inverse=True)
            self.classes_ = np.array(classes)
            return yy

    kw = dict(n_iter=8, random_state=0, max_neurons=16)
    now = SomClassifier(backend=us.UnitStatsOracleBackend(), **kw).fit(X, y)
    was = Before(backend=us.UnitStatsOracleBackend(), **kw).fit(X, y)
    assert np.array_equal(now.classes_, np.unique(y)) and np.array_equal(now.classes_, was.classes_)
    assert np.array_equal(now.weights_, was.weights_) and np.array_equal(now.predict(X), was.predict(X))
    assert set(np.unique(now.predict(X))) <= set(now.classes_)
    vq = SomVQ(backend=us.UnitStatsOracleBackend(), **kw).fit(X, y)
    assert not hasattr(vq, "classes_") and np.array_equal(vq.labels_, vq.predict(X))     # (SomVQ ignores any y)
    assert np.array_equal(vq.weights_, SomVQ(backend=us.UnitStatsOracleBackend(), **kw).fit(X).weights_)
    ent = SomClassifier(growth_criterion="entropy", backend=us.UnitStatsOracleBackend(), **kw).fit(X, y)
    assert np.array_equal(ent.classes_, np.unique(y)) and ent.growing_threshold_ == 0.5


# ---- argument errors of the C ABI -----------------------------------------------------------------------------------
def test_argument_errors_are_status_codes():
    lib = _native.load()
    p = 4096                                                                 # a stand-in address; nothing is dereferenced
    big = _native.MAX_PROTOTYPES + 1
    err = lambda: lib.dbgsom_last_error().decode()                           # noqa: E731
    calls = [
        ("dbgsom_ctx_unit_sums", (None, p, p, None, 10, 4, 2, None, p), "null pointer"),
        ("dbgsom_ctx_unit_sums", (None, None, p, None, 10, 4, 2, p, p), "null pointer"),
        ("dbgsom_ctx_unit_sums", (None, p, p, None, -1, 4, 2, p, p), "N must be"),
        ("dbgsom_ctx_unit_sums", (None, p, p, None, 2 ** 31, 4, 2, p, p), "N must be"),
        ("dbgsom_ctx_unit_sums", (None, p, p, None, 10, 0, 2, p, p), "M must be"),
        ("dbgsom_ctx_unit_sums", (None, p, p, None, 10, big, 2, p, p), "M must be"),
        ("dbgsom_ctx_unit_sums", (None, p, p, None, 10, 4, 0, p, p), "n_values must be"),
        ("dbgsom_ctx_unit_sums", (None, p, p, None, 10, 4, 17, p, p), "n_values must be"),
        ("dbgsom_ctx_unit_sums_device", (None, p, p, 2, None, 10, 4, 2, p, None, 2), "null pointer"),
        ("dbgsom_ctx_unit_sums_device", (None, p, p, 1, None, 10, 4, 2, p, p, 2), "stride of the input"),
        ("dbgsom_ctx_unit_sums_device", (None, p, p, 2, None, 10, 4, 2, p, p, 1), "stride of the output"),
        ("dbgsom_ctx_unit_sums_device", (None, p, p, 2, None, 2 ** 31, 4, 2, p, p, 2), "N must be"),
        ("dbgsom_ctx_unit_sums_device", (None, p, p, 2, None, 10, big, 2, p, p, 2), "M must be"),
        ("dbgsom_ctx_unit_sums_device", (None, p, p, 17, None, 10, 4, 17, p, p, 17), "n_values must be"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, p, 2, 10, p, 2, 4, 2, 2, p, 2), "mode must be"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, p, 2, 10, p, 2, 4, 2, -1, p, 2), "mode must be"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, None, 2, 10, p, 2, 4, 2, 0, p, 2), "null pointer"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, p, 1, 10, p, 2, 4, 2, 0, p, 2), "stride of the input"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, p, 2, 10, p, 1, 4, 2, 1, p, 1), "stride of the input"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, p, 2, 10, p, 2, 4, 2, 0, p, 1), "stride of the output"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, p, 2, -1, p, 2, 4, 2, 0, p, 2), "N must be"),
        ("dbgsom_ctx_unit_deviations_device", (None, p, p, 2, 10, p, 2, 0, 2, 0, p, 2), "M must be"),
        ("dbgsom_ctx_set_targets", (None, p, 10, 0), "n_values must be"),
        ("dbgsom_ctx_set_targets", (None, p, 10, 17), "n_values must be"),
        ("dbgsom_ctx_set_targets_device", (None, None, 10, 2, 2), "null pointer"),
        ("dbgsom_ctx_set_targets_device", (None, p, 10, 1, 2), "ldy below n_values"),
        ("dbgsom_ctx_set_targets_device", (None, p, 10, 17, 17), "n_values must be"),
        ("dbgsom_ctx_target_statistics", (None, None, 4, None, p, None, None), "null pointer"),
        ("dbgsom_ctx_target_statistics", (None, None, 0, p, p, None, None), "M must be"),
        ("dbgsom_ctx_target_statistics", (None, None, big, p, p, None, None), "M must be"),
    ]
    for name, args, word in calls:
        assert getattr(lib, name)(*args) == EINVAL, (name, args)
        assert err().startswith(name + ":") and word in err(), (name, err())
    # with every argument in range the missing context is what is left to report, still before any device work
    assert lib.dbgsom_ctx_unit_sums_device(None, p, p, 2, None, 10, 4, 2, p, p, 2) == EINVAL and "null context" in err()
    assert lib.dbgsom_ctx_unit_deviations_device(None, p, p, 2, 10, p, 2, 4, 2, 1, p, 0) == EINVAL and "null context" in err()
    for name in ("dbgsom_ctx_unit_sums", "dbgsom_ctx_unit_sums_device", "dbgsom_ctx_unit_deviations_device",
                 "dbgsom_ctx_set_targets", "dbgsom_ctx_set_targets_device", "dbgsom_ctx_target_statistics"):
        assert name in _native.SIGNATURES
    with open(_native.HEADER) as f:
        header = f.read()
    assert "#define DBGSOM_ABI_VERSION 4" in header and "#define DBGSOM_DEVIATIONS_NORM 1" in header
    assert (bk.DEVIATIONS_SQUARES, bk.DEVIATIONS_NORM, bk.UNIT_BLOCK) == (0, 1, 128)
