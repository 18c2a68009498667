"""CPU: prototype_density / u_star_matrix -- the helper that turns a radius into a squared threshold, the oracle of the
count down the columns against a plain Python loop and as a fold, the estimator plumbing on a CPU stand-in backend and on
the NumPy default of the base backend with the invariant of the interface, every refusal by its message, the crafted
table holding the cases it claims, and the argument errors of the new ABI calls as status codes."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.exceptions import NotFittedError

from dbgsom_amd import SomClassifier, SomVQ, _native
from dbgsom_amd.backend import HotPathBackend, squared_threshold, squared_thresholds
from tests import density as dn
from tests import distortion as ds
from tests import exemplars as ex
from tests import golden_inputs as gi
from tests import prototype_distances as pd
from tests.test_missing_cpu import punch


# ---- the threshold helper -------------------------------------------------------------------------------------------
def _is_the_largest_under_the_root(rho, t):
    up = np.nextafter(t, np.inf)
    return np.sqrt(t) <= rho and (rho < np.sqrt(up) or t == np.finfo(np.float64).max)


def test_threshold_is_the_largest_square_under_the_radius():
    tiny = 5e-324
    radii = [0.0, tiny, 2 * tiny, 2.0 ** -1074, 2.0 ** -1060, 2.0 ** -1022, 2.2250738585072014e-308, 1e-200,
             1.4916681462400413e-154,                       # around sqrt of the smallest normal number
             1.0, 2.0, 3.0, 4.0, 7.0, 1024.0, 3.0 ** 20,     # perfect squares under the root: t = rho^2 exactly representable
             0.1, 0.3, 1.0 / 3.0, np.pi, np.e, 1.1, 1.3, 1.7, 2.5e-3, 123456.789]
    radii += [float(np.nextafter(r, np.inf)) for r in (1.0, 2.0, 0.1, 1e10)]
    radii += [float(np.nextafter(r, -np.inf)) for r in (1.0, 2.0, 0.1, 1e10)]
    radii += [10.0 ** e for e in range(-160, 151, 10)] + [3.7 * 10.0 ** e for e in range(-160, 150, 31)]
    rng = np.random.default_rng(0)
    radii += list(rng.random(300) * 10.0 ** rng.integers(-160, 150, 300))
    up = down = same = 0
    for rho in radii:
        t = squared_threshold(rho)
        assert isinstance(t, float) and t >= 0.0 and np.isfinite(t)
        assert _is_the_largest_under_the_root(rho, t), (rho, t)
        sq = float(np.float64(rho) * np.float64(rho))
        up, down, same = up + (t > sq), down + (t < sq), same + (t == sq)
    assert up and down and same                             # squares that round up, down and not at all are all met
    assert squared_threshold(0.0) == 0.0 and squared_threshold(tiny) == 0.0
    assert squared_threshold(2.0) == np.nextafter(4.0, 5.0)                      # sqrt(4 + 1 ulp) still rounds to 2
    assert squared_threshold(1e200) == np.finfo(np.float64).max                  # the square overflows
    assert squared_threshold(np.float32(1.5)) == squared_threshold(1.5) and squared_threshold(3) == squared_threshold(3.0)
    got = squared_thresholds([3.0, 0.0, 3.0])
    assert got.dtype == np.float64 and got.flags.c_contiguous and got[0] == got[2] == squared_threshold(3.0) and got[1] == 0.0
    for bad in (np.nan, np.inf, -np.inf, -1.0, -tiny):
        with pytest.raises(ValueError, match="finite and >= 0"):
            squared_threshold(bad)


def test_threshold_turns_the_rooted_comparison_into_a_squared_one():
    rng = np.random.default_rng(1)
    for scale in (1e-150, 1e-3, 1.0, 1e7, 1e140):
        r = rng.random(4000) * scale
        r[:50] = 0.0
        for rho in np.concatenate([np.sqrt(r[100:130]), np.quantile(np.sqrt(r), [0.0, 0.1, 0.5, 1.0])]):
            t = squared_threshold(rho)
            assert np.array_equal(r <= t, np.sqrt(r) <= rho)
            around = np.array([t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf) if t > 0 else 0.0])
            assert np.array_equal(around <= t, np.sqrt(around) <= rho)


# ---- the oracle -----------------------------------------------------------------------------------------------------
ORACLE_CASES = [c for c in dn.COLS_CASES if c[0] <= 300][::4]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[dn.COLS_IDS[dn.COLS_CASES.index(c)] for c in ORACLE_CASES])
def test_oracle_is_a_plain_loop(case):
    N, M, n = case
    R, thr = dn.cols_matrix(case)
    got = dn.range_counts_oracle(R, thr)
    assert got.shape == (M, n) and got.dtype == np.int64
    for j in range(M):
        for t in range(n):
            assert got[j, t] == sum(1 for i in range(N) if float(R[i, j]) <= float(thr[t]))
    cuts = [0, N // 7, N // 7 + (N + 1) // 2, N]                      # three blocks of uneven size (some may be empty)
    parts = sum(dn.range_counts_oracle(R[a:b], thr) for a, b in zip(cuts[:-1], cuts[1:]))
    assert np.array_equal(parts, got)


def test_oracle_on_special_entries():
    inf, nan = np.inf, np.nan
    R = np.array([[0.0, nan, 1.0, inf],
                  [1.0, nan, 1.0, 3.0],
                  [0.0, nan, np.nextafter(1.0, 2.0), nan],
                  [4.0, nan, np.nextafter(1.0, 0.0), 2.0]])
    got = dn.range_counts_oracle(R, [1.0, 0.0, 1.0, nan, inf])
    assert np.array_equal(got, [[3, 2, 3, 0, 4], [0, 0, 0, 0, 0], [3, 0, 3, 0, 4], [0, 0, 0, 0, 3]])


def test_tables_reach_what_they_claim():
    cases = dn.COLS_CASES
    short = [c for c in cases if c not in dn.COLS_LONG]
    assert {c[1] for c in short} == set(dn.COLS_M) and {c[0] for c in short} == set(dn.COLS_N)
    assert {(c[1], c[2]) for c in cases} >= {(M, n) for M in dn.COLS_M for n in dn.COLS_NR}
    assert {dn.r_instance(c[2]) for c in cases} == set(dn.R_INSTANCES)
    assert {1, 2, 3, 5, 31, 32} <= set(dn.COLS_NR)
    assert any(c[2] < dn.r_instance(c[2]) for c in cases)             # padded thresholds
    assert all(dn.segment_rows(c[0], c[1]) == 64 for c in short)
    assert {64 - 1, 64, 64 + 1, 256 - 1, 256, 256 + 1, dn.LOADS - 1, dn.LOADS, dn.LOADS + 1} <= set(dn.COLS_N)
    for RB in (1, 8, 16, 32):                                          # every N: the ends of a segment, a workgroup, the unroll
        assert {c[0] for c in short if dn.r_instance(c[2]) == RB} >= set(dn.COLS_N)
    assert [dn.segment_rows(*c[:2]) for c in dn.COLS_LONG] == [72, 72, 1024]
    assert [c[0] % dn.segment_rows(*c[:2]) for c in dn.COLS_LONG] == [48, 24, 6]
    assert [-(-c[0] // dn.segment_rows(*c[:2])) % 4 for c in dn.COLS_LONG] == [3, 0, 2]      # wavefronts of the last workgroup
    assert [dn.segment_rows(N, M) for N, M in ((8192, 1024), (65536, 100), (100000, 25), (322560, 25))] == [64, 64, 64, 72]
    assert len(cases) < 100 and sum(c[0] * c[1] for c in short) < 3e6 and sum(c[0] * c[1] for c in dn.COLS_LONG) < 2e7
    seen = dict(equal=0, above=0, below=0, zero=0, dup=0, nan_col=0, inf=0, nan_col_m1=0)
    for case in cases:
        N, M, n = case
        R, thr = dn.cols_matrix(case)
        assert R.shape == (N, M) and thr.shape == (n,)
        with np.errstate(invalid="ignore"):
            assert ((R >= 0) | np.isnan(R)).all()
        for t in range(n):
            seen["equal"] += bool((R == thr[t]).any())
            seen["above"] += bool((R == np.nextafter(thr[t], np.inf)).any())
            seen["below"] += bool(thr[t] > 0 and (R == np.nextafter(thr[t], -np.inf)).any())
        if n >= 3:
            assert thr[2] == 0.0 and thr[1] == thr[0]
            seen["zero"] += bool((R[:, 0] == 0.0).any()) or N < 10
            seen["dup"] += 1
        if M >= 3:
            assert np.isnan(R[:, M - 1]).all()
            seen["nan_col"] += 1
            seen["inf"] += bool(np.isposinf(R[:, M - 2]).any())
        elif np.isnan(R).all():
            seen["nan_col_m1"] += 1
        want = dn.range_counts_oracle(R, thr)
        if N >= 3 and M >= 3:
            assert (want.sum(axis=0) >= 1).all()                       # every threshold is met by the entry equal to it
    assert all(v > 0 for v in seen.values()), seen
    assert seen["equal"] >= sum(c[2] for c in cases if c[0] >= 3) * 0.9
    assert dn.SLAB_CASE[1] == 300
    for i in range(len(pd.CASES)):
        assert len(set(dn.case_nr(i))) == 2
    assert {dn.r_instance(n) for i in range(len(pd.CASES)) for n in dn.case_nr(i)} >= {1, 2, 4, 8, 16, 32}


def test_case_radii_count_what_the_rooted_matrix_counts():
    for i in (0, 7, 12, 22):
        case = pd.CASES[i]
        R = ds.case_reference(case)[0]
        for n in dn.case_nr(i):
            radii, thr, counts = dn.case_reference(case, n)
            D = np.sqrt(R)
            assert np.array_equal(counts, np.stack([np.count_nonzero(D <= r, axis=0) for r in radii], axis=1))
            assert counts.max() > 0 and (D.size == 1 or counts.min() < D.shape[0])


# ---- estimator plumbing on the stand-in -----------------------------------------------------------------------------
FIT_KW = dict(random_state=0, n_iter=15, max_neurons=20)


@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=dn.DensityOracleBackend(), **FIT_KW).fit(X)
    return est, X


def _by_the_matrix(est, X, radii):
    D = est.prototype_distances(X)
    return np.stack([np.count_nonzero(D <= r, axis=0) for r in np.atleast_1d(radii)], axis=1).astype(np.int64)


def test_scalar_array_permuted_and_duplicated_radii(fitted):
    est, X = fitted
    be = est._engine()
    be.range_calls = []
    Xq = X[:150]
    M = len(est.weights_)
    D = est.prototype_distances(Xq)
    rho = float(np.median(D))
    one = est.prototype_density(Xq, rho)
    assert isinstance(one, np.ndarray) and one.shape == (M,) and one.dtype == np.int64
    assert np.array_equal(one, _by_the_matrix(est, Xq, rho)[:, 0]) and 0 < one.sum() < D.size
    assert est.density_radius_ == rho
    radii = np.quantile(D, [0.05, 0.3, 0.6, 0.9])
    radii[2] = D[17, 3]                                                # an exact entry: the pair itself is counted
    many = est.prototype_density(Xq, radii)
    assert many.shape == (M, 4) and many.dtype == np.int64
    assert np.array_equal(many, _by_the_matrix(est, Xq, radii))
    assert np.array_equal(est.density_radius_, radii)
    order = [2, 0, 3, 1, 0, 0]                                         # any order, duplicates allowed
    assert np.array_equal(est.prototype_density(Xq, radii[order]), many[:, order])
    assert np.array_equal(est.prototype_density(Xq, list(radii)), many)
    assert np.array_equal(est.prototype_density(Xq, tuple(radii[:1])), many[:, :1])     # one radius in a list: (M, 1)
    assert np.array_equal(est.prototype_density(Xq, np.float32(rho)), est.prototype_density(Xq, float(np.float32(rho))))
    assert np.array_equal(est.prototype_density(Xq, [0, 1000]), np.stack([(D == 0).sum(0), np.full(M, 150)], 1))
    assert np.array_equal(est.prototype_density(Xq, np.arange(32.0)).shape, (M, 32))
    assert [c[0] for c in be.range_calls] == [150] * len(be.range_calls)
    assert np.array_equal(be.range_calls[0][1], squared_thresholds([rho]))
    Xs = np.where(np.abs(Xq) < 2.0, 0.0, Xq).astype(np.float32)
    want = est.prototype_density(Xs, radii)
    for fmt in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        assert np.array_equal(est.prototype_density(fmt(Xs), radii), want)
    Xi = np.rint(Xq[:20]).astype(np.int64)                              # anything but float32 becomes float64, as for predict
    assert np.array_equal(est.prototype_density(Xi, 3.0), est.prototype_density(Xi.astype(np.float64), 3.0))


def test_default_radius_no_rows_and_a_pickle(fitted):
    est, X = fitted
    M = len(est.weights_)
    be = est._engine()
    got = est.prototype_density(X[:200])
    rho = float(est._get_u_matrix().mean())
    assert est.density_radius_ == rho and isinstance(est.density_radius_, float)
    assert np.array_equal(got, _by_the_matrix(est, X[:200], rho)[:, 0]) and got.shape == (M,)
    be.range_calls = []
    for empty in (X[:0], np.empty((0, X.shape[1]))):
        assert np.array_equal(est.prototype_density(empty), np.zeros(M, dtype=np.int64))
        z = est.prototype_density(empty, [1.0, 2.0, 3.0])
        assert z.shape == (M, 3) and z.dtype == np.int64 and not z.any()
    assert be.range_calls == []                                        # no launch
    again = pickle.loads(pickle.dumps(est))
    again.backend = dn.DensityOracleBackend()
    assert np.array_equal(again.prototype_density(X[:200]), got) and again.density_radius_ == rho
    assert np.array_equal(again.u_star_matrix(X[:200]), est.u_star_matrix(X[:200]))


def test_u_star_matrix_is_the_formula(fitted):
    est, X = fitted
    M = len(est.weights_)
    U = est._get_u_matrix()
    for radius in (None, 2.5):
        P = est.prototype_density(X[:300], radius).astype(np.float64)
        got = est.u_star_matrix(X[:300], radius)
        assert isinstance(got, np.ndarray) and got.shape == (M,) and got.dtype == np.float64
        assert P.max() > P.mean()
        scale = (P - P.mean()) / (P.mean() - P.max()) + 1.0
        assert np.array_equal(got, U * scale)
        assert got[np.argmax(P)] == 0.0 and (scale[P < P.mean()] > 1.0).all()
    # max == mean: every unit sees every row, and no row
    assert np.array_equal(est.u_star_matrix(X[:300], 1e6), U)
    assert np.array_equal(est.u_star_matrix(X[:0]), U)
    with pytest.raises(ValueError, match="one radius"):
        est.u_star_matrix(X[:10], [1.0, 2.0])


def test_numpy_default_of_the_base_backend_and_the_classifier():
    X, y = gi.blobs_f32(300, 5, 4, n_centers=3)
    clf = SomClassifier(backend=ex.ExemplarsOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    assert type(clf._engine()).range_counts is HotPathBackend.range_counts           # the stand-in inherits the default
    D = clf.prototype_distances(X[:80])
    radii = np.concatenate([np.quantile(D, [0.1, 0.5]), [D[5, 2], 0.0]])
    got = clf.prototype_density(X[:80], radii)
    assert got.dtype == np.int64 and np.array_equal(got, _by_the_matrix(clf, X[:80], radii))
    own = SomClassifier(backend=dn.DensityOracleBackend(), random_state=0, n_iter=8, max_neurons=12).fit(X, y)
    assert np.array_equal(own.prototype_density(X[:80], radii), got)
    assert own.u_star_matrix(X[:80]).shape == (len(own.weights_),)
    for bad in (np.zeros(0), np.zeros(33)):
        with pytest.raises(ValueError, match="DBGSOM_MAX_RADII"):
            HotPathBackend().range_counts(np.zeros((2, 3)), bad, np.zeros((4, 3)))


def test_refusals_and_their_messages(fitted):
    est, X = fitted
    with pytest.raises(NotFittedError):
        SomVQ(backend=dn.DensityOracleBackend()).prototype_density(X)
    call = est.prototype_density
    with pytest.raises(ValueError, match="X has 5 features, but SomVQ is expecting 8 features as input"):
        call(X[:10, :5])
    with pytest.raises(ValueError, match="features"):
        call(sp.csr_matrix(X[:10, :5]))
    with pytest.raises(ValueError, match="features"):
        call(np.empty((0, 3)))
    for bad in (True, np.True_, "2", b"2", np.nan, np.inf, -np.inf, -1.0, [], np.zeros(0), [1.0, np.nan], [1.0, -2.0],
                [np.inf], [[1.0, 2.0]], np.ones((2, 2)), [True, False], ["a"], 1 + 2j, {"r": 1}):
        with pytest.raises(ValueError, match="radius must be None, a finite real number >= 0 or a 1-D array-like"):
            call(X[:10], radius=bad)
    with pytest.raises(ValueError, match="33 radii are above the 32 .*prototype_distances"):
        call(X[:10], radius=np.arange(33.0))
    assert call(X[:10], radius=np.arange(32.0)).shape[1] == 32
    with pytest.raises(ValueError, match="NaN"):
        call(punch(X[:40], 0.3, 3))
    for missing in ("nan", "nan-fit"):
        holes = SomVQ(backend=dn.DensityOracleBackend(), missing_values=missing, **FIT_KW).fit(X)
        assert holes.prototype_density(X[:10], 2.0).shape == (len(holes.weights_),)
        with pytest.raises(ValueError, match="impute them first"):
            holes.prototype_density(punch(X[:40], 0.3, 3))
        with pytest.raises(ValueError, match="impute them first"):
            holes.u_star_matrix(punch(X[:40], 0.3, 3))
    for metric, label in (("manhattan", "Manhattan"), ("cosine", "cosine")):
        other = SomVQ(backend=dn.DensityOracleBackend(), **FIT_KW)
        other.__dict__.update(est.__dict__)
        other.metric = metric
        for fn in (other.prototype_density, other.u_star_matrix):
            with pytest.raises(ValueError, match=r"metric='%s' \(%s\) does not support prototype_density.*squared Euclidean"
                                                 % (metric, label)):
                fn(X[:10])


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    err = lambda: lib.dbgsom_last_error()   # noqa: E731
    one = 16                                # any non-null aligned address: argument errors come before any device work
    assert _native.MAX_RADII == dn.MAX_RADII == 32
    assert "#define DBGSOM_MAX_RADII 32" in open(_native.HEADER).read()

    fold = lambda N=10, M=5, ldr=5, n=2, p=one, t=one, c=one: lib.dbgsom_range_count_cols(p, N, M, ldr, t, n, c, None)  # noqa: E731
    assert fold(M=0, ldr=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert fold(M=_native.MAX_PROTOTYPES + 1, ldr=20000) == -1 and b"MAX_PROTOTYPES" in err()
    assert fold(n=0) == -1 and b"n_radii" in err()
    assert fold(n=33) == -1 and b"MAX_RADII" in err()
    assert fold(ldr=4) == -1 and b"ldr" in err()
    assert fold(N=-1) == -1 and b"shape" in err()
    assert fold(N=2 ** 31) == -1 and b"shape" in err()
    assert fold(p=None) == -1 and b"null pointer" in err()
    assert fold(t=None) == -1 and b"null pointer" in err()
    assert fold(c=None) == -1 and b"null pointer" in err()
    assert fold(p=20) == -1 and b"aligned" in err()
    assert fold(t=20) == -1 and b"aligned" in err()
    assert fold(c=20) == -1 and b"aligned" in err()
    assert fold(N=0, p=None, t=None, c=None) == 0                     # no rows: the counts stay what they are

    assert lib.dbgsom_range_counts_workspace_bytes(0, 5, 0) == 0 and lib.dbgsom_range_counts_workspace_bytes(10, 0, 0) == 0
    for N, M, slab in ((10, 5, 0), (1000, 70, 0), (1000, 70, 100), (100000, 1024, 0), (300, 33, 7)):
        assert lib.dbgsom_range_counts_workspace_bytes(N, M, slab) == lib.dbgsom_kneighbors_workspace_bytes(N, M, slab)
    need = lib.dbgsom_range_counts_workspace_bytes(10, 5, 0)
    assert need == (10 * 6 * 8 + 255) // 256 * 256                    # one slab, rows M rounded up to even apart
    full = lambda dt=0, N=10, d=4, ldx=4, M=5, n=2, slab=0, p=one, t=one, c=one, w=one, ws=need: (   # noqa: E731
        lib.dbgsom_range_counts(p, dt, N, d, ldx, p, p, M, p, t, n, slab, c, w, ws, None))
    assert full(dt=7) == -1 and b"x_dtype" in err()
    assert full(ldx=3) == -1 and b"shape" in err()
    assert full(N=-1) == -1 and b"shape" in err()
    assert full(M=0) == -1 and b"MAX_PROTOTYPES" in err()
    assert full(n=0) == -1 and b"n_radii" in err()
    assert full(n=33) == -1 and b"MAX_RADII" in err()
    assert full(slab=-1) == -1 and b"slab_rows" in err()
    assert full(p=None) == -1 and b"null pointer" in err()
    assert full(t=None) == -1 and b"null pointer" in err()
    assert full(c=None) == -1 and b"null pointer" in err()
    assert full(w=None) == -1 and b"null pointer" in err()
    assert full(N=0, c=None) == -1 and b"null pointer" in err()       # no rows still stores zeros
    assert full(c=20) == -1 and b"aligned" in err()
    assert full(t=20) == -1 and b"aligned" in err()
    assert full(w=24) == -1 and b"16-byte aligned" in err()
    assert full(ws=need - 1) == -3 and (b"%d bytes, %d needed" % (need - 1, need)) in err()

    W = np.zeros((5, 4))
    out = np.zeros(64)
    w = W.ctypes.data
    calls = (("dbgsom_ctx_range_counts_query", lambda c, M, n, t=one: (c, one, 0, 10, 4, w, M, t, n, one)),
             ("dbgsom_ctx_range_counts_query_device", lambda c, M, n, t=one: (c, one, 0, 10, 4, 4, w, M, t, n, one)),
             ("dbgsom_ctx_range_counts_query_csr", lambda c, M, n, t=one: (c, one, one, one, 0, 10, 4, 3, w, M, t, n, one)))
    for name, args in calls:
        assert getattr(lib, name)(*args(None, 5, 2)) == -1 and b"null context" in err()
        with pytest.raises(ValueError, match="null context"):
            _native.call(name, *args(None, 5, 2))
        assert getattr(lib, name)(*args(out.ctypes.data, 0, 2)) == -1 and b"MAX_PROTOTYPES" in err()   # (before the context is touched)
        assert getattr(lib, name)(*args(out.ctypes.data, 5, 0)) == -1 and b"n_radii" in err()
        assert getattr(lib, name)(*args(out.ctypes.data, 5, 33)) == -1 and b"MAX_RADII" in err()
    assert lib.dbgsom_ctx_range_counts_query(out.ctypes.data, one, 0, 10, 4, w, 5, None, 2, one) == -1 and b"null pointer" in err()
    assert lib.dbgsom_ctx_range_counts_query_device(out.ctypes.data, one, 0, 10, 4, 3, w, 5, one, 2, one) == -1 and b"ldx" in err()
