"""CPU: fit on rows with missing entries (``missing_values="nan-fit"``) -- the NumPy restatement of the masked epoch
against the complete-data oracle and a literal loop, the estimator plumbing on a CPU stand-in backend (start rows,
moments, epoch order, refusals, clone / get_params / pickle, the classifier), and the argument errors of the new
device-level calls as status codes."""
import inspect
import math
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.base import clone

from dbgsom_amd import SomClassifier, SomVQ, _native, schedule
from dbgsom_amd.backend import HotPathBackend
from oracle import som_oracle as o
from tests import device_abi as da
from tests import golden_inputs as gi
from tests import masked_fit as mf
from tests.test_missing_cpu import MaskedOracleBackend, case, masked_bmu, punch


def holes_input(seed=11):
    """blobs with 20 % of the cells punched out, every third row complete -> (X, Xn, labels)"""
    X, lab = gi.blobs_f32(600, 8, 2, n_centers=6)
    Xn = punch(X, 0.2, seed)
    Xn[::3] = X[::3]
    return X, Xn, lab


@pytest.fixture(scope="module")
def fitted():
    X, Xn, _ = holes_input()
    est = SomVQ(backend=mf.MaskedFitOracleBackend(), missing_values="nan-fit", random_state=0, n_iter=15,
                max_neurons=20).fit(Xn)
    return est, X, Xn


# ---- 1. the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,M", [(257, 17, 5), (1000, 64, 129)])
def test_oracle_on_complete_rows_is_the_aligned_update(N, d, M):
    X, W, _ = case(N, d, M, 0.3, "float64")
    X = np.where(np.isnan(X), 0.25, X)                      # complete rows
    hop = gi.lattice_hops(1, M).astype(np.float64)
    tv = np.var(X, axis=0).sum()
    gamma = float(tv ** -1)
    dist, win = o.bmu_chain(X, W, 1)
    kw = o.exp_similarity_gamma(dist, gamma)
    S, K, A, a, E = mf.masked_sums(X, win, kw, dist, M)
    assert np.array_equal(A, np.repeat(a[:, None], d, axis=1))
    S0, K0, a0, E0 = o.accumulate(X, win, kw, dist, M)
    assert np.array_equal(a, a0)
    (Sr, Kr, _, Er), (TS, TK, TE) = da.accumulate_reference(X, win, kw, dist, M)
    for got, ref, T in ((S, Sr, TS), (S0, Sr, TS), (K[:, 0], Kr, TK), (K0, Kr, TK), (E, Er, TE), (E0, Er, TE)):
        ok, ratio = da.sums_within_bound(got, ref, T, a, False)
        assert ok, ratio
    out = mf.masked_epoch(X, W, hop, 1.7, gamma, winners=win, distances=dist)
    want = o.smooth_matmul(o.gaussian_neighborhood(hop, 1.7), a0, o.voronoi_centers(S0, K0, a0, "aligned"))
    np.testing.assert_allclose(out.new_weights, want, rtol=mf.W_RTOL, atol=mf.W_ATOL)


def test_oracle_is_the_literal_triple_loop():
    X, W, _ = case(7, 3, 2, 0.3, "float64")
    N, d, M = 7, 3, 2
    hop = np.array([[0.0, 1.0], [1.0, 0.0]])
    sigma, gamma = 0.9, 0.05
    out = mf.masked_epoch(X, W, hop, sigma, gamma)
    dist, win = masked_bmu(X, W, 1)
    assert np.array_equal(out.winners, win) and np.array_equal(out.distances, dist)
    kw = 1 - np.sqrt(1 - np.exp(-gamma * dist ** 2))
    S, K, A = np.zeros((M, d)), np.zeros((M, d)), np.zeros((M, d))
    a, E = np.zeros(M), np.zeros(M)
    for i in range(N):
        a[win[i]] += 1
        E[win[i]] += dist[i]
        for c in range(d):
            if not np.isnan(X[i, c]):
                S[win[i], c] += kw[i] * X[i, c]
                K[win[i], c] += kw[i]
                A[win[i], c] += 1
    assert all(np.array_equal(g, w) for g, w in zip(out.sums, (S, K, A)))
    assert np.array_equal(out.errors, E) and np.array_equal(out.activations, a)
    Wn = np.array(W, dtype=np.float64)
    for j in range(M):
        for c in range(d):
            num = den = 0.0
            for l in range(M):
                if A[l, c] > 0:
                    h = np.exp(-(hop[j, l] ** 2 / (2 * sigma ** 2)))
                    num += h * A[l, c] * (S[l, c] / K[l, c])
                    den += h * A[l, c]
            if den > 0:
                Wn[j, c] = num / den
    np.testing.assert_allclose(out.new_weights, Wn, rtol=1e-14, atol=0)
    assert out.change_total == pytest.approx(np.linalg.norm(W - out.new_weights, axis=1).sum(), rel=1e-14)


def test_oracle_keeps_an_entry_nobody_in_reach_observed():
    S, K, A, a, E, hop, W_old, sigma = mf.smooth_case(4, 3, split=True)
    Wn = mf.masked_smooth(S, K, A, hop, sigma, W_old)
    assert np.array_equal(Wn[2:, 0], W_old[2:, 0]) and not np.array_equal(Wn[:2, 0], W_old[:2, 0])
    assert np.isfinite(Wn).all()


# ---- 2. the estimator on the stand-in: fails without the feature --------------------------------------------------
def test_fit_on_rows_with_holes(fitted):
    est, X, Xn = fitted
    be = est._engine()
    assert be.masked_epochs >= 1 and be.masked_calls >= 1
    assert np.isfinite(est.weights_).all()
    dist, win = masked_bmu(Xn, est.weights_, 1)
    assert np.array_equal(est.labels_, win)
    assert est.quantization_error_ == float(np.mean(dist))
    assert set(np.unique(win)) == set(range(len(est.weights_)))        # every neuron left has hits
    assert 0.0 <= est.topographic_error_ <= 1.0
    assert est.n_features_in_ == 8


# ---- 3. start rows, moments, gamma and the epoch order ------------------------------------------------------------
def test_fit_without_growth_is_the_hand_written_loop():
    _, Xn, _ = holes_input()
    n_iter = 12
    est = SomVQ(backend=mf.MaskedFitOracleBackend(), missing_values="nan-fit", random_state=0, n_iter=n_iter,
                max_neurons=4).fit(Xn)
    rng = np.random.default_rng(seed=0)
    start = Xn[rng.choice(len(Xn), size=4, replace=False)]
    fill = np.nanmean(Xn, axis=0, dtype=np.float64).astype(Xn.dtype)
    W = np.where(np.isnan(start), fill[None, :], start)
    tv = np.nanvar(Xn, axis=0).sum()
    gamma = float(tv ** -1)
    hop = est._distance_matrix
    assert hop.shape == (4, 4) and sorted(hop[0].tolist()) == [0.0, 1.0, 1.0, 2.0]      # the 2 x 2 lattice
    converged, phase, consumed = False, "coarse", None
    for epoch in range(n_iter):
        if epoch > 0.5 * n_iter:
            phase = "fine"
        sigma = schedule.current_sigma(epoch=epoch, n_neurons=4, n_iter=n_iter, phase=phase,
                                       decay_function="exponential", learning_rate=0.02, coarse_training_frac=0.5,
                                       sigma_start=None, sigma_end=None)
        out = mf.masked_epoch(Xn, W, hop, sigma, gamma)
        consumed, W = W, out.new_weights
        converged = converged or out.change_total < 1e-5
        if converged and phase == "fine":
            break
    assert len(est.weights_) == 4
    assert np.array_equal(est.weights_, np.asarray(W, dtype=np.float64))
    assert est.growing_threshold_ == float(150 * -math.log(0.5) * np.linalg.norm(np.nanstd(Xn, axis=0, ddof=1)))


# ---- 4. complete X ------------------------------------------------------------------------------------------------
def test_complete_rows_take_the_ordinary_path():
    X, _, _ = holes_input()
    be = mf.MaskedFitOracleBackend()
    est = SomVQ(backend=be, missing_values="nan-fit", random_state=0, n_iter=15, max_neurons=20).fit(X)
    plain = SomVQ(backend=MaskedOracleBackend(), random_state=0, n_iter=15, max_neurons=20).fit(X)
    assert be.masked_epochs == 0 and be.masked_calls == 0
    assert np.array_equal(est.weights_, plain.weights_) and np.array_equal(est.labels_, plain.labels_)
    assert est.quantization_error_ == plain.quantization_error_


# ---- 5. imputation ------------------------------------------------------------------------------------------------
def test_imputation_beats_the_column_means(fitted):
    est, X, Xn = fitted
    filled = est.impute(Xn)
    assert not np.isnan(filled).any()
    got, base = mf.impute_rmse(X, Xn, filled), mf.mean_fill_rmse(X, Xn)
    print(f"RMSE over the punched cells: impute {got:.4f}, column means {base:.4f}")
    assert got < base


# ---- 6. refusals and plumbing -------------------------------------------------------------------------------------
def new(**kw):
    kw.setdefault("missing_values", "nan-fit")
    return SomVQ(backend=mf.MaskedFitOracleBackend(), random_state=0, n_iter=5, max_neurons=12, **kw)


def test_refusals():
    X, Xn, lab = holes_input()
    inf = Xn.copy()
    inf[3, 2] = np.inf
    with pytest.raises(ValueError, match="inf"):
        new().fit(inf)
    empty = Xn.copy()
    empty[17] = np.nan
    with pytest.raises(ValueError, match="row 17 .*no observed"):
        new().fit(empty)
    thin = Xn.copy()
    thin[1:, 5] = np.nan
    with pytest.raises(ValueError, match="column 5 "):
        new().fit(thin)
    with pytest.raises(ValueError, match="sample_weight"):
        new().fit(Xn, sample_weight=np.ones(len(Xn)))
    with pytest.raises(ValueError, match="vertical_growth"):
        new(vertical_growth=True).fit(Xn)
    with pytest.raises(ValueError, match="sharded_input"):
        new(sharded_input=True).fit(Xn)
    stored_nan = sp.csr_matrix(np.where(np.isnan(Xn), 0, Xn).astype(np.float64))
    stored_nan.data[5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        new().fit(stored_nan)
    with pytest.raises(ValueError, match="NaN"):                 # "nan" opens the queries only
        new(missing_values="nan").fit(Xn)
    with pytest.raises(ValueError, match="NaN"):
        new(missing_values=None).fit(Xn)
    with pytest.raises(ValueError, match="missing_values"):
        new(missing_values="bogus").fit(X)
    # complete X: none of the refusals of the incomplete mode applies
    new(vertical_growth=True).fit(X)
    with pytest.raises(NotImplementedError):
        HotPathBackend().epoch_masked(np.zeros((2, 2)), np.zeros((2, 2)), 1.0, 1.0)


def test_parameter_survives_clone_pickle_and_get_params(fitted):
    est, X, Xn = fitted
    assert list(inspect.signature(SomVQ.__init__).parameters)[-1] == "missing_values"
    c = clone(est)
    assert c.missing_values == "nan-fit" and c.get_params()["missing_values"] == "nan-fit"
    back = pickle.loads(pickle.dumps(est))
    assert back.missing_values == "nan-fit"
    back.backend = back._backend_obj = mf.MaskedFitOracleBackend()
    q = punch(X[:50], 0.3, 1)
    assert np.array_equal(back.predict(q), est.predict(q))


def test_queries_equal_those_under_nan(fitted):
    est, X, _ = fitted
    other = pickle.loads(pickle.dumps(est))
    other.missing_values = "nan"
    other.backend = other._backend_obj = MaskedOracleBackend()
    q = punch(X[:120], 0.3, 2)
    q[::4] = X[:120:4]
    assert np.array_equal(est.predict(q), other.predict(q))
    assert est.calculate_quantization_error(q) == other.calculate_quantization_error(q)
    assert np.array_equal(est.impute(q), other.impute(q))
    assert np.array_equal(est.transform(q), other.transform(q))
    with pytest.raises(ValueError, match="NaN"):
        est.topographic_function(q)


@pytest.mark.parametrize("criterion", ["quantization_error", "entropy"])
def test_classifier(criterion):
    X, Xn, lab = holes_input()
    y = lab % 3
    be = mf.MaskedFitOracleBackend()
    clf = SomClassifier(backend=be, missing_values="nan-fit", random_state=0, n_iter=12, max_neurons=16,
                        growth_criterion=criterion).fit(Xn, y)
    assert be.masked_epochs >= 1 and np.isfinite(clf.weights_).all()
    q = punch(X[:60], 0.3, 5)
    pred = clf.predict(q)
    assert pred.shape == (60,) and set(pred) <= set(np.unique(y))
    assert np.array_equal(clf.predict_proba(q), clf.predict_proba(clf.impute(q)), equal_nan=True)
    assert (clf.predict(Xn) == y).mean() > 0.5


# ---- 7. the ABI's argument errors, without a GPU ------------------------------------------------------------------
def test_abi_argument_errors_are_status_codes():
    lib = _native.load()
    p = 1 << 20              # (a non-null, 256-byte aligned address that is never dereferenced: the checks come first)
    F32, F64, BF16 = _native.F32, _native.F64, _native.BF16
    need = lib.dbgsom_accumulate_masked_workspace_bytes(10, 4, 5)
    assert need >= 10 * 4 + 5 * (3 * 4 + 2) * 8 and lib.dbgsom_accumulate_masked_workspace_bytes(10, 0, 5) == 0
    acc = lib.dbgsom_accumulate_masked
    assert acc(p, F64, 10, 0, 4, p, p, p, 5, p, p, p, need, None) == -1           # d < 1
    assert b"bad sample shape" in lib.dbgsom_last_error()
    assert acc(p, F64, 10, 4, 3, p, p, p, 5, p, p, p, need, None) == -1           # ldx < d
    assert b"bad sample shape" in lib.dbgsom_last_error()
    assert acc(p, BF16, 10, 4, 4, p, p, p, 5, p, p, p, need, None) == -1
    assert b"x_dtype" in lib.dbgsom_last_error()
    assert acc(p, F32, 10, 4, 4, p, p, p, 0, p, p, p, need, None) == -1           # M < 1
    for null_at in (0, 5, 6, 7, 11):                                               # X, idx, kw, dist, workspace
        args = [p, F32, 10, 4, 4, p, p, p, 5, p, p, p, need, None]
        args[null_at] = None
        assert acc(*args) == -1 and b"null pointer" in lib.dbgsom_last_error()
    assert acc(p, F32, 10, 4, 4, p, p, p, 5, None, p, p, need, None) == -1
    assert b"null sums" in lib.dbgsom_last_error()
    assert acc(p, F32, 10, 4, 4, p, p, p, 5, p, p, p, need - 1, None) == -3
    assert b"workspace" in lib.dbgsom_last_error()
    sm = lib.dbgsom_smooth_masked
    sneed = lib.dbgsom_smooth_masked_workspace_bytes(5, 4)
    assert sneed > 0 and lib.dbgsom_smooth_masked_workspace_bytes(0, 4) == 0
    assert sm(p, 5, 0, p, 1.0, p, p + 4096, p, p, sneed, None) == -1               # d < 1
    assert b"bad shape" in lib.dbgsom_last_error()
    assert sm(None, 5, 4, p, 1.0, p, p + 4096, p, p, sneed, None) == -1
    assert b"null pointer" in lib.dbgsom_last_error()
    assert sm(p, 5, 4, p, 1.0, p, p, p, p, sneed, None) == -1
    assert b"alias" in lib.dbgsom_last_error()
    assert sm(p, 5, 4, p, 0.0, p, p + 4096, p, p, sneed, None) == -1
    assert b"sigma" in lib.dbgsom_last_error()
    assert sm(p, 5, 4, p, 1.0, p, p + 4096, p, p, sneed - 1, None) == -3
    assert b"workspace" in lib.dbgsom_last_error()
    with pytest.raises(ValueError, match="x_dtype"):
        _native.call("dbgsom_accumulate_masked", p, BF16, 10, 4, 4, p, p, p, 5, p, p, p, need, None)
    assert lib.dbgsom_ctx_bmu_masked(None, p, 5, 1, p, p) == -1                    # null context
    assert lib.dbgsom_ctx_epoch_masked(None, p, 5, 1.0, 1.0, p, p, p, p, None, None) == -1
