"""CPU: queries on rows with missing entries (NaN) -- the NumPy oracle of the masked distance, its inputs, the
estimator plumbing (split and scatter, refusals, ``impute``, composition with the coder, clone / get_params /
pickle) on a CPU stand-in backend, and the argument errors of the new ABI calls as status codes.

The oracle and the inputs are also imported by tests/test_gpu_missing.py."""
import copy
import functools
import inspect
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.base import clone

from dbgsom_amd import SomClassifier, SomVQ, _native
from oracle import som_oracle as o
from tests import golden_inputs as gi

# Tolerance on distances against the oracle, derived (not measured): a float64 sum of n <= 4096 non-negative
# terms with <= 2 roundings each is off by at most about (n + 2) 1.1e-16 < 5e-13 relative, whatever the order
# of summation; the scale adds two roundings, the square root halves the total.
RTOL = 1e-12
GAP = 1e-9   # required relative gap between the 1st and 2nd, and the 2nd and 3rd, smallest oracle distance of a row

SHAPES = [(1, 1, 1), (7, 3, 2), (257, 17, 5), (1000, 64, 129), (1000, 130, 300), (513, 784, 260)]
FRACS = [0.0, 0.3, 0.9]
DTYPES = [np.float32, np.float64]
GRID = [(N, d, M, frac, dt) for (N, d, M) in SHAPES for frac in FRACS for dt in DTYPES]
GRID_IDS = [f"{N}x{d}x{M}-{frac}-{np.dtype(dt).name}" for (N, d, M, frac, dt) in GRID]


# ---- oracle ---------------------------------------------------------------------------------------------------
def masked_distances(X, W, rows_at_a_time=None):
    """(N x M) float64: sqrt(d / n_obs * sum over the observed k of (x_k - w_k)^2), direct form."""
    X = np.asarray(X)
    X64 = X.astype(np.float64)           # (float32 is widened exactly)
    W64 = np.asarray(W, dtype=np.float64)
    N, d = X64.shape
    obs = ~np.isnan(X64)
    n_obs = obs.sum(axis=1)
    if (n_obs == 0).any():
        raise ValueError(f"row {int(np.argmax(n_obs == 0))} of X has no observed entry")
    step = rows_at_a_time or max(1, (1 << 23) // max(1, W64.shape[0] * d))
    out = np.empty((N, W64.shape[0]))
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        diff = np.where(obs[lo:hi, None, :], X64[lo:hi, None, :] - W64[None, :, :], 0.0)
        out[lo:hi] = np.sqrt((diff ** 2).sum(axis=2) * (d / n_obs[lo:hi])[:, None])
    return out


def masked_bmu(X, W, k=1):
    """-> (dist, idx) in ``bmu``'s shapes: lexicographic minimum on (distance, index)."""
    D = masked_distances(X, W)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(D, idx, axis=1)
    if k == 1:
        return dist.reshape(-1), idx.reshape(-1)
    return dist, idx


def fill_numpy(X, W, idx):
    """X with every NaN replaced by that entry of W[idx[row]], cast to X's dtype."""
    out = np.array(X, copy=True)
    holes = np.isnan(out)
    out[holes] = np.asarray(W, dtype=np.float64)[np.asarray(idx).reshape(len(out), -1)[:, 0]][holes].astype(out.dtype)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------
def make_case(N, d, M, frac, dtype):
    """8 centres C = 3 N(0, 1); W = C[random] + N(0, 1) (float64); X = C[random] + N(0, 1) cast to dtype; one
    random cell per row is kept, every other cell is punched out with probability frac.  frac = 0: exactly one
    NaN in the whole array, at row N // 2 in the last column (none when d = 1: the row's only cell stays)."""
    rng = np.random.default_rng(1000 * N + 10 * d + M + int(10 * frac))
    C = 3.0 * rng.standard_normal((8, d))
    W = C[rng.integers(0, 8, M)] + rng.standard_normal((M, d))
    X = (C[rng.integers(0, 8, N)] + rng.standard_normal((N, d))).astype(dtype)
    keep = rng.integers(0, d, N)
    if frac > 0:
        holes = rng.random((N, d)) < frac
        holes[np.arange(N), keep] = False
        X[holes] = np.nan
    elif d > 1:
        X[N // 2, d - 1] = np.nan
    return X, W


@functools.lru_cache(maxsize=None)
def case(N, d, M, frac, dtype_name):
    """-> (X, W, D): the inputs and the oracle's distance matrix, computed once and shared (read only)."""
    X, W = make_case(N, d, M, frac, np.dtype(dtype_name).type)
    D = masked_distances(X, W)
    for a in (X, W, D):
        a.setflags(write=False)
    return X, W, D


def smallest_gap(D):
    """Smallest relative gap between the 1st and 2nd, and the 2nd and 3rd, smallest distance of a row."""
    if D.shape[1] < 2:
        return np.inf
    S = np.sort(D, axis=1)[:, :3]
    return float(((S[:, 1:] - S[:, :-1]) / S[:, 1:]).min())


def winners_of(D, k):
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(D, idx, axis=1)
    return (dist.reshape(-1), idx.reshape(-1)) if k == 1 else (dist, idx)


def punch(X, frac, seed):
    """A copy of X with cells set to NaN with probability frac, one random cell per row kept."""
    rng = np.random.default_rng(seed)
    X = np.array(X, copy=True)
    holes = rng.random(X.shape) < frac
    holes[np.arange(len(X)), rng.integers(0, X.shape[1], len(X))] = False
    X[holes] = np.nan
    return X


# ---- CPU stand-in backend -------------------------------------------------------------------------------------
class MaskedOracleBackend(o.OracleBackend):
    """OracleBackend with ``bmu_masked`` in NumPy (TESTS ONLY, like its base class); counts its masked calls."""

    def __init__(self, bmu="chain"):
        super().__init__(bmu)
        self.masked_calls = 0
        self.bmu_rows = []

    def bmu(self, W, k=1, X=None):
        if X is not None:
            self.bmu_rows.append(len(X))
            assert not np.isnan(X).any()
        return super().bmu(W, k, X)

    def bmu_masked(self, W, k, X, want_filled=False):
        self.masked_calls += 1
        dist, idx = masked_bmu(X, W, k)
        return (dist, idx, fill_numpy(X, W, idx)) if want_filled else (dist, idx)


# ---- the oracle and its inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,M,frac,dt", GRID, ids=GRID_IDS)
def test_inputs_meet_the_gap_condition(N, d, M, frac, dt):
    X, W, D = case(N, d, M, frac, np.dtype(dt).name)
    assert X.dtype == dt and X.shape == (N, d) and W.shape == (M, d)
    n_nan = int(np.isnan(X).sum())
    assert (n_nan == (1 if d > 1 else 0)) if frac == 0 else (d == 1 or n_nan > 0)
    assert not np.isnan(X).all(axis=1).any()
    if frac == 0.9 and d in (3, 17):
        assert ((~np.isnan(X)).sum(axis=1) == 1).any()     # rows of a single observed cell
    gap = smallest_gap(D)
    print(f"smallest relative gap {gap:.2e}")
    assert gap > GAP


def test_oracle_against_nan_euclidean_distances():
    """scikit-learn's function uses the expanded form |x|^2 - 2 x.w + |w|^2 on zero-filled rows and then takes the
    missing entries' share of |w|^2 off again, so the bound is ITS accuracy: the squared distance carries an
    absolute error of a few eps (|x_O|^2 + |w|^2) d / n_obs, x_O the row's observed entries and w the WHOLE
    prototype (each term is a float64 sum of <= d products; 2 (d + 2) eps covers their roundings and the
    additions and subtractions between them).  Largest error seen here, as a fraction of that bound: WORST."""
    from sklearn.metrics.pairwise import nan_euclidean_distances

    eps = np.finfo(np.float64).eps
    worst = 0.0
    for (N, d, M) in [(7, 3, 2), (257, 17, 5), (1000, 64, 129)]:
        for frac in FRACS:
            X, W, D = case(N, d, M, frac, "float64")
            S = nan_euclidean_distances(X, W)
            obs = ~np.isnan(X)
            scale = d / obs.sum(axis=1)
            xx = (np.where(obs, X, 0.0) ** 2).sum(axis=1)
            ww = (W ** 2).sum(axis=1)
            bound = 2 * (d + 2) * eps * scale[:, None] * (xx[:, None] + ww[None, :])
            err = np.abs(S ** 2 - D ** 2)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all()
    print(f"largest |sklearn^2 - oracle^2| / bound = {worst:.2e}")


def test_oracle_edge_semantics():
    W = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [1.0, 2.0, 3.0]])
    X = np.array([[1.0, np.nan, 3.0], [np.nan, 2.0, np.nan], [0.0, 0.0, 0.0]])
    dist, idx = masked_bmu(X, W, 2)
    assert dist[0, 0] == 0.0 and dist[0, 1] == 0.0 and idx[0].tolist() == [0, 2]   # duplicates: lowest index first
    assert dist[1, 0] == 0.0 and idx[1].tolist() == [0, 1]
    assert np.allclose(dist[2], np.sqrt([14.0, 14.0]))                              # a complete row: plain distance
    with pytest.raises(ValueError, match="row 1 .*no observed"):
        masked_distances(np.array([[1.0, 2.0], [np.nan, np.nan]]), W[:, :2])


# ---- estimator plumbing on the stand-in ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    X, _ = gi.blobs_f32(600, 8, 2, n_centers=6)
    est = SomVQ(backend=MaskedOracleBackend(), missing_values="nan", random_state=0, n_iter=15, max_neurons=20).fit(X)
    return est, X


def test_parameter_is_validated_on_first_use_and_survives_clone_and_pickle(fitted):
    est, X = fitted
    assert SomVQ().missing_values is None and "missing_values" in SomVQ().get_params()
    assert list(inspect.signature(SomVQ.__init__).parameters)[-1] == "missing_values"   # behind the existing ones
    bogus = SomVQ(backend=MaskedOracleBackend(), missing_values="bogus", n_iter=3)   # (no error in __init__)
    with pytest.raises(ValueError, match="missing_values"):
        bogus.fit(X)
    c = clone(est)
    assert c.missing_values == "nan" and c.get_params()["missing_values"] == "nan"
    back = pickle.loads(pickle.dumps(est))
    assert back.missing_values == "nan"
    back.backend = back._backend_obj = MaskedOracleBackend()
    Xn = punch(X[:50], 0.3, 1)
    assert np.array_equal(back.predict(Xn), est.predict(Xn))


def test_split_and_scatter(fitted):
    est, X = fitted
    be = est._engine()
    Xn = punch(X[:200], 0.3, 2)
    Xn[::3] = X[:200:3]                                   # every third row complete
    incomplete = np.isnan(Xn).any(axis=1)
    be.masked_calls, be.bmu_rows = 0, []
    labels = est.predict(Xn)
    assert be.masked_calls == 1 and be.bmu_rows == [int((~incomplete).sum())]
    want = masked_bmu(Xn, est.weights_, 1)
    assert np.array_equal(labels, want[1])                # (the oracle on complete rows is the plain argmin)
    plain = SomVQ(backend=MaskedOracleBackend(), random_state=0, n_iter=15, max_neurons=20).fit(X)
    assert np.array_equal(plain.weights_, est.weights_)   # the parameter changes nothing about fit
    assert np.array_equal(labels[~incomplete], plain.predict(Xn[~incomplete]))
    qe = est.calculate_quantization_error(Xn)
    dist = np.empty(len(Xn))
    dist[incomplete] = want[0][incomplete]
    dist[~incomplete] = plain._get_winning_neurons(Xn[~incomplete], 1)[0]
    assert qe == float(np.mean(dist))
    # k = 2 keeps bmu's shapes
    d2, i2 = est._get_winning_neurons(Xn, 2)
    assert d2.shape == i2.shape == (200, 2) and np.array_equal(i2[incomplete], masked_bmu(Xn[incomplete], est.weights_, 2)[1])
    # no incomplete row: no masked call at all
    be.masked_calls = 0
    assert np.array_equal(est.predict(X[:100]), plain.predict(X[:100])) and be.masked_calls == 0


def test_refusals(fitted):
    est, X = fitted
    Xn = punch(X[:40], 0.3, 3)
    with pytest.raises(ValueError, match="NaN"):      # fit takes complete rows only, under both settings
        SomVQ(backend=MaskedOracleBackend(), missing_values="nan", random_state=0, n_iter=5).fit(
            np.vstack([Xn, X[40:80]]))
    with pytest.raises(ValueError, match="NaN"):
        SomVQ(backend=MaskedOracleBackend(), random_state=0, n_iter=5).fit(np.vstack([Xn, X[40:80]]))
    plain = SomVQ(backend=MaskedOracleBackend(), random_state=0, n_iter=15, max_neurons=20).fit(X)
    for call in (plain.predict, plain.calculate_quantization_error, plain.transform):
        with pytest.raises(ValueError, match="NaN"):
            call(Xn)
    with pytest.raises(ValueError, match="missing_values='nan'"):
        plain.impute(Xn)
    empty = Xn.copy()
    empty[17] = np.nan
    for call in (est.predict, est.calculate_quantization_error, est.impute, est.transform):
        with pytest.raises(ValueError, match="row 17 .*no observed"):
            call(empty)
    inf = Xn.copy()
    inf[3, 2] = np.inf
    for call in (est.predict, est.calculate_quantization_error, est.impute, est.transform):
        with pytest.raises(ValueError, match="inf"):
            call(inf)
    stored_nan = sp.csr_matrix(np.where(np.isnan(Xn), 0, Xn).astype(np.float64))
    stored_nan.data[5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        est.predict(stored_nan)
    with pytest.raises((TypeError, ValueError)):
        est.impute(sp.csr_matrix(X[:10].astype(np.float64)))
    with pytest.raises(ValueError, match="NaN"):
        est.topographic_function(Xn)                      # keeps refusing
    bogus = copy.copy(est)
    bogus.missing_values = "bogus"
    with pytest.raises(ValueError, match="missing_values"):
        bogus.predict(Xn)


@pytest.mark.parametrize("dt", DTYPES)
def test_impute(fitted, dt):
    est, X = fitted
    Xn = punch(X[:120], 0.4, 4).astype(dt)
    Xn[::4] = X[:120:4].astype(dt)
    before = Xn.copy()
    out = est.impute(Xn)
    assert out.dtype == dt and out is not Xn and np.array_equal(Xn, before, equal_nan=True)   # input untouched
    holes = np.isnan(Xn)
    assert not np.isnan(out).any()
    assert np.array_equal(out[~holes], Xn[~holes])                                           # observed: bitwise
    idx = masked_bmu(Xn, est.weights_, 1)[1]
    assert np.array_equal(out[holes], est.weights_.astype(np.float64)[idx][holes].astype(dt))
    assert est.impute(Xn.tolist()).dtype == np.float64                                        # validated dtype
    full = X[:30].astype(dt)
    got = est.impute(full)
    assert got is not full and np.array_equal(got, full)


def test_classifier_composition():
    X, lab = gi.blobs_f32(600, 8, 2, n_centers=6)
    y = lab % 3
    clf = SomClassifier(backend=MaskedOracleBackend(), missing_values="nan", random_state=0, n_iter=15,
                        max_neurons=20).fit(X, y)
    Xn = punch(X[:60], 0.3, 5)
    filled = clf.impute(Xn)
    assert np.array_equal(clf.predict_proba(Xn), clf.predict_proba(filled), equal_nan=True)
    assert np.array_equal(clf.predict(Xn), clf.predict(filled))
    assert np.array_equal(clf.transform(Xn), clf.transform(filled))
    plain = SomClassifier(backend=MaskedOracleBackend(), random_state=0, n_iter=15, max_neurons=20).fit(X, y)
    assert np.array_equal(plain.predict_proba(X[:60]), clf.predict_proba(X[:60]), equal_nan=True)
    with pytest.raises(ValueError, match="NaN"):
        plain.predict_proba(Xn)
    clf.vertical_growth = True                             # (the branch is taken on the flag alone)
    with pytest.raises(ValueError, match="vertical_growth"):
        clf.predict_proba(Xn)


def test_base_backend_has_no_masked_search():
    from dbgsom_amd.backend import HotPathBackend

    with pytest.raises(NotImplementedError):
        HotPathBackend().bmu_masked(np.zeros((2, 2)), 1, np.zeros((1, 2)))
    with pytest.raises(NotImplementedError):
        o.OracleBackend().bmu_masked(np.zeros((2, 2)), 1, np.zeros((1, 2)))


# ---- the ABI's argument errors, without a GPU -----------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    one = np.zeros(1)
    p = one.ctypes.data      # (a non-null pointer that is never dereferenced: the checks come first)
    F32, F64, BF16 = _native.F32, _native.F64, _native.BF16
    # k = 3
    assert lib.dbgsom_bmu_masked(p, F64, 10, 4, 4, p, 5, 4, 3, p, p, p, 1 << 20, None) == -1
    assert b"k must be 1 or 2" in lib.dbgsom_last_error()
    # bfloat16 rows
    assert lib.dbgsom_bmu_masked(p, BF16, 10, 4, 4, p, 5, 4, 1, p, p, p, 1 << 20, None) == -1
    assert b"x_dtype" in lib.dbgsom_last_error()
    assert lib.dbgsom_fill_missing(p, BF16, 10, 4, 4, p, 5, 4, p, 1, None) == -1
    assert b"x_dtype" in lib.dbgsom_last_error()
    # M < k
    assert lib.dbgsom_bmu_masked(p, F32, 10, 4, 4, p, 1, 4, 2, p, p, p, 1 << 20, None) == -1
    assert b"k <= M" in lib.dbgsom_last_error()
    # null pointers
    assert lib.dbgsom_bmu_masked(None, F32, 10, 4, 4, p, 5, 4, 1, p, p, p, 1 << 20, None) == -1
    assert b"null pointer" in lib.dbgsom_last_error()
    assert lib.dbgsom_bmu_masked(p, F32, 10, 4, 4, p, 5, 4, 1, p, None, p, 1 << 20, None) == -1
    assert b"null pointer" in lib.dbgsom_last_error()
    assert lib.dbgsom_fill_missing(p, F32, 10, 4, 4, None, 5, 4, p, 1, None) == -1
    assert b"null pointer" in lib.dbgsom_last_error()
    # a workspace that is too small is found before any launch as well
    need = lib.dbgsom_bmu_masked_workspace_bytes(F32, 10, 4, 5)
    assert need >= 4 * 256 * 8 + 10 * 4 + 10 * 4 * 8
    assert lib.dbgsom_bmu_masked_workspace_bytes(F64, 10, 4, 5) < need      # no float64 copy of float64 rows
    assert lib.dbgsom_bmu_masked(p, F32, 10, 4, 4, p, 5, 4, 1, p, p, p, need - 1, None) == -3
    assert b"workspace" in lib.dbgsom_last_error()
    with pytest.raises(ValueError, match="k must be 1 or 2"):
        _native.call("dbgsom_bmu_masked", p, F64, 10, 4, 4, p, 5, 4, 3, p, p, p, 1 << 20, None)
