"""CPU: the map as a Gaussian mixture -- the restatement of the rows kernel of csrc/mixture.hip against np.longdouble,
against scipy's logsumexp and scikit-learn's GaussianMixture, its exact cases bit for bit, the host default of the
backend, the estimator plumbing on a CPU stand-in backend, every refusal by its message, and the argument errors of the
new ABI calls as status codes."""
import math
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.special import logsumexp
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd.backend import HotPathBackend, mixture_rows_host
from tests import device_abi as da
from tests import distortion as ds
from tests import golden_inputs as gi
from tests import mixture as mx
from tests import prototype_distances as pd
from tests.test_missing_cpu import punch


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


# ---- the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not da.have_longdouble(), reason="np.longdouble has no 64-bit significand here")
@pytest.mark.parametrize("case", mx.ROWS_CASES, ids=mx.ROWS_IDS)
def test_restatement_is_within_its_bound_of_the_longdouble_sums(case):
    N, M, nv, equal = case
    R, a, c, Y = mx.rows_problem(case)
    b, lse, q, S, Q, T = mx.mixture_rows(R, a, c, Y, parts=True)
    Sr, Qr, Ar, lr = mx.longdouble_parts(R, a, c, Y, b)
    rows = mx.defined(R, a, c)
    B = mx.bound(M, mx.E_NP)
    L = np.longdouble
    assert (np.abs(S[rows].astype(L) - Sr[rows]) <= B * Sr[rows]).all()
    assert (np.abs(Q[rows].astype(L) - Qr[rows]) <= B * Qr[rows]).all()          # (Y > 0: A == Q)
    assert (np.abs(lse[rows].astype(L) - lr[rows]) <= B + 2 * mx.U * np.abs(lr[rows])).all()
    worst = mx.check_outputs(R, a, c, Y, b, lse, q, mx.E_NP)
    print("%s: largest error / bound: lse %.3f, q %.3f" % (mx.ROWS_IDS[mx.ROWS_CASES.index(case)], *worst))
    assert np.isnan(lse[~rows]).all() and np.isnan(q[~rows]).all()


def test_restatement_on_special_rows():
    inf, nan = np.inf, np.nan
    R = np.array([[4.0, 1.0, nan, 1.0, inf, 0.25],      # a NaN: the unit from the others, lse and q NaN
                  [nan, nan, nan, nan, nan, nan],       # nothing: (-1, NaN, NaN)
                  [2.0, 1.0, 1.0, 3.0, inf, 5.0],       # equal maxima: the lowest index; +inf: s = 0
                  [2.0, 1.0, 1.0, 3.0, 7.0, 5.0]])
    a = np.full(6, -np.log(6.0))
    Y = np.arange(12.0).reshape(6, 2)
    b, lse, q = mx.mixture_rows(R, a, 1.0, Y)
    assert np.array_equal(b, [5, -1, 1, 1])
    assert np.isnan(lse[:2]).all() and np.isnan(q[:2]).all() and np.isfinite(lse[2:]).all() and np.isfinite(q[2:]).all()
    gone = np.array([0.0, -inf, -inf, 0.0, -inf, -inf])                  # units without mass are never the unit
    b, lse, q = mx.mixture_rows(R, gone, 1.0, Y)
    assert np.array_equal(b, [3, -1, 0, 0]) and np.isnan(lse[0]) and lse[3] == -2.0 + np.log(1.0 + np.exp(-1.0))
    b, lse, q = mx.mixture_rows(R, np.full(6, -inf), 1.0, Y)             # no unit has mass
    assert (b == -1).all() and np.isnan(lse).all() and np.isnan(q).all()
    b, lse, q = mx.mixture_rows(R[3:], a, 1.0, None)
    assert q.shape == (1, 0) and b[0] == 1


def test_against_scipy_logsumexp_and_sklearn_gaussian_mixture():
    from sklearn.mixture import GaussianMixture

    rng = np.random.default_rng(5)
    n, d, M = 200, 7, 13
    X, W = rng.normal(size=(n, d)), rng.normal(size=(M, d))
    w = rng.random(M) + 0.1
    w /= w.sum()
    h = 0.8
    R = ds.squared_matrix(X, W)
    Y = rng.normal(size=(M, 3))
    b, lse, q = mx.mixture_rows(R, np.log(w), 1.0 / (2 * h * h), Y)
    logp = lse - 0.5 * d * math.log(2 * math.pi * h * h)
    exact = ((X[:, None, :] - W[None]) ** 2).sum(axis=2)
    t = np.log(w)[None] - exact / (2 * h * h)
    assert np.max(np.abs(logp - (logsumexp(t, axis=1) - 0.5 * d * math.log(2 * math.pi * h * h)))) <= 1e-10
    gm = GaussianMixture(n_components=M, covariance_type="spherical")
    gm.weights_, gm.means_, gm.covariances_ = w, W, np.full(M, h * h)
    gm.precisions_cholesky_ = np.full(M, 1.0 / h)
    assert np.max(np.abs(logp - gm.score_samples(X))) <= 1e-10
    assert np.array_equal(b, gm.predict(X))
    assert np.max(np.abs(q - gm.predict_proba(X) @ Y)) <= 1e-10


# ---- exact cases: nothing here depends on anyone's exp ---------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 257, 300])
def test_exact_cases_on_the_restatement(M):
    rng = np.random.default_rng(M)
    N, V = 5, 3
    R = rng.random((N, M)) * 10.0 + 1e-3
    a = np.full(M, -np.log(M))
    Y = rng.normal(size=(M, V))
    # c = 0 with equal priors: every s_j = 1, S = M, q the fixed-order column mean
    b, lse, q, S, Q, T = mx.mixture_rows(R, a, 0.0, Y, parts=True)
    assert (b == 0).all() and (S == float(M)).all() and (T == a[0]).all()
    mean = np.array([mx.lane_sum(Y[:, v]) / float(M) for v in range(V)])
    assert np.array_equal(_bits(q), _bits(np.tile(mean, (N, 1))))
    assert np.array_equal(_bits(lse), _bits(np.full(N, a[0] + np.log(float(M)))))
    # c so large that every s_j but the winner's is 0: S = 1, q = Y[b], lse = T
    c = mx.underflow_c(R)
    b, lse, q, S, Q, T = mx.mixture_rows(R, a, c, Y, parts=True)
    assert np.array_equal(b, np.argmin(R, axis=1)) and (S == 1.0).all()
    assert np.array_equal(_bits(q), _bits(Y[b])) and np.array_equal(_bits(lse), _bits(T))
    assert np.array_equal(_bits(T), _bits(a[0] - c * R[np.arange(N), b]))
    # Y all ones: q = 1 wherever S is finite
    for cc in (0.0, 0.7, c):
        b, lse, q = mx.mixture_rows(R, a, cc, np.ones((M, 2)))
        assert (q == 1.0).all()


def test_tables_reach_what_they_claim():
    assert {c[0] for c in mx.ROWS_CASES} == set(mx.ROWS_N) and {c[1] for c in mx.ROWS_CASES} == set(mx.ROWS_M)
    assert {c[2] for c in mx.ROWS_CASES} == set(mx.ROWS_NV)
    assert {mx.v_instance(c[2]) for c in mx.ROWS_CASES} == set(mx.V_INSTANCES)
    assert {(c[1], c[3]) for c in mx.ROWS_CASES} == {(M, e) for M in mx.ROWS_M for e in (True, False)}
    kinds = set()
    for case in mx.ROWS_CASES:
        N, M, nv, equal = case
        R, a, c, Y = mx.rows_problem(case)
        b, lse, q = mx.mixture_rows(R, a, c, Y)
        assert Y.shape == (M, nv) and (Y > 0).all()
        if N >= mx.ROWS_KINDS:
            if equal:
                assert b[0] == 0 and b[1] == (63 if M > 63 else 0)
            assert b[2] == -1 and np.isnan(lse[2]) and np.isnan(q[2]).all()
            assert M < 3 or (np.isposinf(R[3]).any() and np.isfinite(lse[3]))
            assert M == 1 or (b[4] >= 0 and np.isnan(lse[4]))
            kinds.add((M > 64, equal))
        if not equal and M >= 3:
            assert np.isneginf(a).any()
    assert (True, True) in kinds                         # ties at lanes 0 / 63 / 64 under equal priors
    assert mx.SLAB_CASE in pd.CASES and mx.SLAB_CASE[1] == 300
    assert {mx.case_nv(i) for i in range(len(pd.CASES))} == set(mx.ROWS_NV)


# ---- the backend's host default -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mx.ROWS_CASES[::3], ids=mx.ROWS_IDS[::3])
def test_host_restatement_of_the_backend_is_the_same_arithmetic(case):
    R, a, c, Y = mx.rows_problem(case)
    b, lse, q = mx.mixture_rows(R, a, c, Y)
    hb, hl, hq = mixture_rows_host(R, a, c, Y if Y.shape[1] else None)
    assert np.array_equal(hb, b) and np.array_equal(_bits(hl), _bits(lse))
    if Y.shape[1]:
        assert np.array_equal(_bits(hq), _bits(q))
    else:
        assert hq is None


def test_base_backend_default_runs_on_its_distances():
    class OnlyDistances(HotPathBackend):
        def distances(self, W, X):
            return np.sqrt(ds.squared_matrix(X, W))

    rng = np.random.default_rng(2)
    X, W = rng.normal(size=(50, 6)), rng.normal(size=(9, 6))
    a = np.full(9, -np.log(9.0))
    Y = rng.random((9, 2))
    b, lse, q = OnlyDistances().mixture(W, a, 0.5, Y, X)
    wb, wl, wq = mx.mixture_rows(ds.squared_matrix(X, W), a, 0.5, Y)
    assert np.array_equal(b, wb)
    np.testing.assert_allclose(lse, wl, rtol=0, atol=1e-12)
    np.testing.assert_allclose(q, wq, rtol=0, atol=1e-12)
    assert OnlyDistances().mixture(W, a, 0.5, None, X)[2] is None
    for bad, msg in (((W, a[:4], 0.5, Y, X), "log_prior must be"), ((W, a, -1.0, Y, X), "c must be >= 0"),
                     ((W, a, np.nan, Y, X), "c must be >= 0"), ((W, a, 0.5, Y[:4], X), "Y must be"),
                     ((W, a, 0.5, np.ones((9, 17)), X), "DBGSOM_MAX_MIXTURE_VALUES = 16")):
        with pytest.raises(ValueError, match=msg):
            OnlyDistances().mixture(*bad)
    with pytest.raises(NotImplementedError):
        HotPathBackend().mixture(W, a, 0.5, Y, X)


# ---- estimator plumbing on the stand-in -----------------------------------------------------------------------------
FIT_KW = dict(random_state=0, n_iter=15, max_neurons=20)


@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=mx.MixtureOracleBackend(), **FIT_KW).fit(X)
    return est, X


def test_fit_mixture_from_host_and_csr(fitted):
    est, X = fitted
    M, d = len(est.weights_), X.shape[1]
    before = {k: np.array(v) for k, v in est.__dict__.items() if isinstance(v, np.ndarray)}
    assert est.fit_mixture(X) is est
    for k, v in before.items():
        assert np.array_equal(getattr(est, k), v), k                     # nothing fit set has moved
    dist, idx = est.kneighbors(X, 1)
    assert est.mixture_priors_.shape == (M,) and est.mixture_priors_.dtype == np.float64
    assert np.array_equal(est.mixture_priors_, np.bincount(idx[:, 0], minlength=M) / 600.0)
    assert abs(est.mixture_priors_.sum() - 1.0) <= 1e-12
    h2 = math.fsum(float(v) * float(v) for v in dist[:, 0]) / (600 * d)
    assert est.mixture_bandwidth_ == math.sqrt(h2) and isinstance(est.mixture_bandwidth_, float)
    h, priors = est.mixture_bandwidth_, est.mixture_priors_.copy()
    perm = np.random.default_rng(0).permutation(600)
    assert est.fit_mixture(X[perm]).mixture_bandwidth_ == h              # fsum: the order does not matter
    assert np.array_equal(est.mixture_priors_, priors)
    Xz = np.where(np.abs(X) < 1.0, 0.0, X).astype(np.float32)
    hz, pz = est.fit_mixture(Xz).mixture_bandwidth_, est.mixture_priors_.copy()
    assert est.fit_mixture(sp.csr_matrix(Xz)).mixture_bandwidth_ == hz
    assert np.array_equal(est.mixture_priors_, pz)
    assert est.fit_mixture(X, bandwidth=0.75).mixture_bandwidth_ == 0.75
    assert np.array_equal(est.mixture_priors_, priors)
    est.fit_mixture(X)
    back = pickle.loads(pickle.dumps(est))
    assert back.mixture_bandwidth_ == h and np.array_equal(back.mixture_priors_, priors)
    with pytest.raises(ValueError, match="not a finite value > 0"):
        est2 = SomVQ(backend=mx.MixtureOracleBackend(), **FIT_KW)
        est2.__dict__.update(est.__dict__)
        est2.fit_mixture(np.ascontiguousarray(est.weights_[:3], dtype=np.float64))   # every row on a prototype: h = 0
    est.fit_mixture(X)


def test_score_samples_and_friends(fitted):
    est, X = fitted
    est.fit_mixture(X)
    M, d = len(est.weights_), X.shape[1]
    h = est.mixture_bandwidth_
    Q = X[:120]
    be = est._engine()
    be.mixture_calls.clear()
    logp = est.score_samples(Q)
    assert logp.shape == (120,) and logp.dtype == np.float64
    n, a, c, Y = be.mixture_calls[-1]
    assert n == 120 and Y is None and c == 1.0 / (2.0 * h * h)
    with np.errstate(divide="ignore"):
        assert np.array_equal(a, np.log(est.mixture_priors_))
    wb, wl, _ = mx.mixture_rows(ds.squared_matrix(Q, est.weights_), a, c)
    assert np.array_equal(_bits(logp), _bits(wl - 0.5 * d * math.log(2 * math.pi * h * h)))
    ld, unit = est.sample_mixture(Q)
    assert np.array_equal(_bits(ld), _bits(logp)) and np.array_equal(unit, wb) and unit.dtype == np.int64
    assert est.calculate_log_likelihood(Q) == float(np.sum(logp)) / 120
    assert isinstance(est.calculate_log_likelihood(Q), float)
    # uniform priors: the MAP unit is the best matching unit
    _, unit_u = est.sample_mixture(Q, priors="uniform")
    assert np.array_equal(unit_u, est.predict(Q))
    assert np.array_equal(be.mixture_calls[-1][1], np.log(np.full(M, 1.0 / M)))
    # arguments override the attributes
    est.score_samples(Q, bandwidth=2.0, priors=np.full(M, 1.0 / M))
    assert be.mixture_calls[-1][2] == 0.125
    # the projection
    pos = est.project(Q)
    nodes = np.asarray(list(est.neurons_), dtype=np.float64)
    assert pos.shape == (120, 2) and pos.dtype == np.float64
    assert (pos >= nodes.min(axis=0) - 1e-12).all() and (pos <= nodes.max(axis=0) + 1e-12).all()
    assert np.array_equal(be.mixture_calls[-1][3], nodes)
    sharp = est.project(Q, bandwidth=1e-3, priors="uniform")             # a tiny bandwidth: onto the unit's node
    assert np.array_equal(sharp, nodes[est.predict(Q)])
    # posterior means
    vals = np.random.default_rng(1).random((M, 5))
    pm = est.posterior_mean(Q, vals)
    assert pm.shape == (120, 5)
    assert np.array_equal(_bits(pm), _bits(mx.mixture_rows(ds.squared_matrix(Q, est.weights_), a, c, vals)[2]))
    flat = est.posterior_mean(Q, vals[:, 2])
    assert flat.shape == (120,) and np.allclose(flat, pm[:, 2], rtol=0, atol=1e-14)
    assert (est.posterior_mean(Q, np.ones(M)) == 1.0).all()
    assert est.posterior_mean(Q, np.ones((M, 16))).shape == (120, 16)
    # CSR rows: the dense result
    Xz = np.where(np.abs(Q) < 1.0, 0.0, Q).astype(np.float32)
    assert np.array_equal(_bits(est.score_samples(sp.csr_matrix(Xz))), _bits(est.score_samples(Xz)))
    # no rows: no call
    calls = len(be.mixture_calls)
    empty = np.empty((0, d), dtype=np.float32)
    assert est.score_samples(empty).shape == (0,) and est.project(empty).shape == (0, 2)
    assert est.sample_mixture(empty)[1].dtype == np.int64 and len(be.mixture_calls) == calls
    with pytest.raises(ValueError, match="0 sample"):
        est.calculate_log_likelihood(empty)
    with pytest.raises(ValueError, match="0 sample"):
        est.fit_mixture(empty)


def test_classifier_inherits_the_calls_and_keeps_score():
    X, y = gi.blobs_f32(300, 6, 3, n_centers=3)
    clf = SomClassifier(backend=mx.MixtureOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    clf.fit_mixture(X)
    assert clf.score_samples(X[:20]).shape == (20,)
    assert 0.0 <= clf.score(X, y) <= 1.0                                 # ClassifierMixin.score: the accuracy
    M = len(clf.weights_)
    onehot = np.eye(3)[np.random.default_rng(0).integers(0, 3, M)]
    shares = clf.posterior_mean(X[:20], onehot)
    np.testing.assert_allclose(shares.sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_refusals_and_their_messages(fitted):
    est, X = fitted
    est.fit_mixture(X)
    M = len(est.weights_)
    calls = {"fit_mixture": est.fit_mixture, "score_samples": est.score_samples, "sample_mixture": est.sample_mixture,
             "calculate_log_likelihood": est.calculate_log_likelihood, "project": est.project,
             "posterior_mean": lambda Z, **kw: est.posterior_mean(Z, np.ones(M), **kw)}
    for name in calls:
        with pytest.raises(NotFittedError):
            fresh = SomVQ(backend=mx.MixtureOracleBackend())
            getattr(fresh, name)(X, np.ones(3)) if name == "posterior_mean" else getattr(fresh, name)(X)
    for name, call in calls.items():
        with pytest.raises(ValueError, match="X has 5 features, but SomVQ is expecting 8 features as input"):
            call(X[:10, :5])
        with pytest.raises(ValueError, match="features"):
            call(sp.csr_matrix(X[:10, :5]))
        with pytest.raises(ValueError, match="NaN"):
            call(punch(X[:40], 0.3, 3))
        with pytest.raises(ValueError, match="[Ii]nf"):
            call(np.where(np.isnan(punch(X[:40], 0.3, 3)), np.inf, X[:40]))
        for bad in (0, 0.0, -1.0, np.inf, np.nan, "2", True, [1.0], 1e-200):
            with pytest.raises(ValueError, match="bandwidth must be None or a finite float > 0"):
                call(X[:10], bandwidth=bad)
    for name, call in calls.items():
        if name == "fit_mixture":
            continue
        for bad, msg in (("flat", "priors must be None, 'uniform' or an array-like"),
                         (np.ones(M + 1) / (M + 1), "priors must be None, 'uniform' or an array-like"),
                         (np.ones((M, 1)) / M, "priors must be None, 'uniform' or an array-like"),
                         (np.ones(M), "sum to 1 within 1e-9"),
                         (np.r_[-0.5, 1.5, np.zeros(M - 2)], "finite and non-negative"),
                         (np.r_[np.nan, np.ones(M - 1)], "finite and non-negative")):
            with pytest.raises(ValueError, match=msg):
                call(X[:10], priors=bad)
        p = np.zeros(M)
        p[0], p[1] = 0.5, 0.5 + 5e-10
        call(X[:10], priors=p)                                            # within 1e-9 of 1
    bare = SomVQ(backend=mx.MixtureOracleBackend(), **FIT_KW)
    bare.__dict__.update({k: v for k, v in est.__dict__.items() if not k.startswith("mixture_")})
    for call in (bare.score_samples, bare.sample_mixture, bare.calculate_log_likelihood, bare.project):
        with pytest.raises(ValueError, match="fit_mixture"):
            call(X[:10])
        with pytest.raises(ValueError, match="fit_mixture"):
            call(X[:10], bandwidth=1.0)                                   # still no priors
        with pytest.raises(ValueError, match="fit_mixture"):
            call(X[:10], priors="uniform")                                # still no bandwidth
    assert bare.score_samples(X[:10], bandwidth=1.0, priors="uniform").shape == (10,)
    stale = SomVQ(backend=mx.MixtureOracleBackend(), **FIT_KW)
    stale.__dict__.update(est.__dict__)
    stale.mixture_priors_ = np.ones(M + 2) / (M + 2)
    with pytest.raises(ValueError, match="fit_mixture"):
        stale.score_samples(X[:10])
    for bad, msg in ((np.ones((M, 17)), "17 columns, above the 16"), (np.ones(M - 1), "values must have shape"),
                     (np.ones((M, 2, 2)), "values must have shape"), (np.ones((M, 0)), "values must have shape"),
                     ("abc", "values must be real numbers")):
        with pytest.raises(ValueError, match=msg):
            est.posterior_mean(X[:10], bad)
    for missing in ("nan", "nan-fit"):
        holes = SomVQ(backend=mx.MixtureOracleBackend(), missing_values=missing, **FIT_KW).fit(X)
        assert holes.fit_mixture(X[:50]).score_samples(X[:10]).shape == (10,)
        for call in (holes.fit_mixture, holes.score_samples, holes.sample_mixture, holes.calculate_log_likelihood,
                     holes.project, lambda Z: holes.posterior_mean(Z, np.ones(len(holes.weights_)))):
            with pytest.raises(ValueError, match="impute them first"):
                call(punch(X[:40], 0.3, 3))
    for metric, label in (("manhattan", "Manhattan"), ("cosine", "cosine")):
        other = SomVQ(backend=mx.MixtureOracleBackend(), **FIT_KW)
        other.__dict__.update(est.__dict__)
        other.metric = metric
        for call in (other.fit_mixture, other.score_samples, other.sample_mixture, other.calculate_log_likelihood,
                     other.project, lambda Z: other.posterior_mean(Z, np.ones(M))):
            with pytest.raises(ValueError, match=r"metric='%s' \(%s\) does not support .*Gaussian in the Euclidean distance"
                                                 % (metric, label)):
                call(X[:10])


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()   # noqa: E731
    one = 16                                # any non-null aligned address: argument errors come before any device work
    assert _native.MAX_MIXTURE_VALUES == mx.MAX_VALUES == 16

    def rows(N=10, M=5, ldr=5, c=1.0, nv=2, ldy=2, ldq=2, p=one, a=one, y=one, q=one):
        return lib.dbgsom_mixture_rows(p, N, M, ldr, a, c, y, nv, ldy, p, p, q, ldq, None)

    assert rows(M=0, ldr=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert rows(M=_native.MAX_PROTOTYPES + 1, ldr=20000) == -1 and b"MAX_PROTOTYPES" in err()
    assert rows(ldr=4) == -1 and b"ldr" in err()
    assert rows(nv=-1) == -1 and b"n_values" in err()
    assert rows(nv=17, ldy=17, ldq=17) == -1 and b"DBGSOM_MAX_MIXTURE_VALUES" in err()
    assert rows(ldy=1) == -1 and b"ldy" in err()
    assert rows(ldq=1) == -1 and b"ldq" in err()
    assert rows(c=-1.0) == -1 and b"c must be >= 0" in err()
    assert rows(c=float("nan")) == -1 and b"c must be >= 0" in err()
    assert rows(N=-1) == -1 and b"shape" in err()
    for kw in (dict(p=None), dict(a=None), dict(y=None), dict(q=None)):
        assert rows(**kw) == -1 and b"null pointer" in err()
    for kw in (dict(p=20), dict(a=20), dict(y=20), dict(q=20)):
        assert rows(**kw) == -1 and b"aligned" in err()
    assert rows(N=0, p=None, a=None, y=None, q=None) == 0          # no rows: nothing to do, nothing dereferenced

    need = lib.dbgsom_kneighbors_workspace_bytes(10, 5, 0)      # (the slab of dbgsom_kneighbors: no size function of its own)
    assert need > 0

    def full(dt=0, N=10, d=4, ldx=4, M=5, c=1.0, nv=2, ldy=2, ldq=2, slab=0, p=one, a=one, y=one, q=one, w=one, ws=need):
        return lib.dbgsom_mixture(p, dt, N, d, ldx, p, p, M, p, a, c, y, nv, ldy, slab, p, p, q, ldq, w, ws, None)

    assert full(dt=7) == -1 and b"x_dtype" in err()
    assert full(ldx=3) == -1 and b"shape" in err()
    assert full(M=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert full(nv=17, ldy=17, ldq=17) == -1 and b"n_values" in err()
    assert full(ldy=1) == -1 and b"ldy" in err()
    assert full(ldq=1) == -1 and b"ldq" in err()
    assert full(c=-0.5) == -1 and b"c must be >= 0" in err()
    assert full(slab=-1) == -1 and b"slab_rows" in err()
    for kw in (dict(p=None), dict(a=None), dict(y=None), dict(q=None), dict(w=None)):
        assert full(**kw) == -1 and b"null pointer" in err()
    assert full(a=20) == -1 and b"aligned" in err()
    assert full(w=24) == -1 and b"16-byte aligned" in err()
    assert full(ws=need - 1) == -3 and (b"%d bytes, %d needed" % (need - 1, need)) in err()
    assert full(N=0, p=None, a=None, y=None, q=None, w=None, ws=0) == 0

    W = np.zeros((5, 4))
    a5 = np.zeros(5)
    for fn, head in (("dbgsom_ctx_mixture_query", lambda N, d: (None, one, 0, N, d)),
                     ("dbgsom_ctx_mixture_query_device", lambda N, d: (None, one, 0, N, d, d)),
                     ("dbgsom_ctx_mixture_query_csr", lambda N, d: (None, one, one, one, 0, N, d, 0))):
        call = getattr(lib, fn)
        assert call(*head(10, 4), W.ctypes.data, 5, a5.ctypes.data, 1.0, None, 0, one, one, None) == -1
        assert b"null context" in err() and fn.encode() in err()
