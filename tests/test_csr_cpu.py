"""CPU: the host side of sparse input -- validation, the column moments from the stored entries, the start rows,
chunked sparse coding, vertical growth on CSR row selections -- with a CPU stand-in backend (the oracle's, its
``load`` / ``bmu`` densifying CSR; the oracle itself stays dense), and ``dbgsom_csr_check`` (host only)."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.base import clone

from dbgsom_amd import SomClassifier, SomVQ, _native
from oracle import som_oracle as o


class CsrOracleBackend(o.OracleBackend):
    """OracleBackend that takes CSR where HipBackend does, by densifying it, and honours ``set_sample_weight``
    like tests/test_sample_weight_cpu.py's stand-in (TESTS ONLY, like its base class)."""

    def load(self, X):
        return super().load(X.toarray() if sp.issparse(X) else X)

    def bmu(self, W, k=1, X=None):
        return super().bmu(W, k, X.toarray() if X is not None and sp.issparse(X) else X)

    def _local_sums(self, W, gamma, want_assignments):
        dist, win = self._fn(self._X, np.asarray(W), 1)
        sums = self._sums_from(W, o.exp_similarity_gamma(dist, gamma), win, dist)
        return sums, (win if want_assignments else None), (dist if want_assignments else None)

    def _sums_from(self, W, sample_weights, winners, distances):
        if self._sw is None:
            return super()._sums_from(W, sample_weights, winners, distances)
        M, keep, w = np.asarray(W).shape[0], self._sw > 0, self._sw
        S, K, _, E = o.accumulate(self._X[keep], winners[keep], (w * sample_weights)[keep], (w * distances)[keep], M)
        return self._pack(S, K, np.bincount(winners, weights=w, minlength=M), E)


# ---- test data (also imported by tests/test_gpu_csr.py) ----------------------------------------------------
def digits_csr(dtype=np.float64):
    from sklearn.datasets import load_digits

    dg = load_digits()
    return sp.csr_matrix(dg.data.astype(dtype)), dg.target


def topics(N=3000, d=2048, dtype=np.float64, seed=3, empty_rows=0, stored_zeros=0, unused_tail=0):
    """10 topics of min(120, d // 10) columns each; per row the distinct columns among 30 draws from its topic's
    columns plus 6 from all columns (less `unused_tail` columns at the end that nobody uses), gamma(2, 1) values:
    about 32 stored entries per row.  `empty_rows` rows are emptied, `stored_zeros` stored values set to 0 (they
    stay stored).  -> (csr, topic of every row)"""
    rng = np.random.default_rng(seed)
    width = min(120, d // 10)
    topic = rng.integers(0, 10, N)
    cols_used = d - unused_tail
    rows, cols = [], []
    for i in range(N):
        c = np.unique(np.r_[topic[i] * width + rng.integers(0, width, 30), rng.integers(0, cols_used, 6)])
        rows.append(np.full(c.size, i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.gamma(2.0, 1.0, rows.size).astype(dtype)
    if stored_zeros:
        vals[rng.choice(vals.size, stored_zeros, replace=False)] = 0
    if empty_rows:
        keep = ~np.isin(rows, rng.choice(N, empty_rows, replace=False))
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    X = sp.csr_matrix((vals, (rows, cols)), shape=(N, d))   # (keeps the explicit zeros)
    assert X.has_canonical_format
    return X, topic


def uncanonical(X, seed=5):
    """The same matrix with the entries of every row shuffled and some of them split into two stored entries
    (duplicates whose sum is the original value exactly: halves)."""
    rng = np.random.default_rng(seed)
    coo = X.tocoo()
    split = rng.random(coo.nnz) < 0.1
    r = np.r_[coo.row, coo.row[split]]
    c = np.r_[coo.col, coo.col[split]]
    v = np.r_[np.where(split, coo.data / 2, coo.data), coo.data[split] / 2]
    perm = rng.permutation(r.size)
    order = np.argsort(r[perm], kind="stable")     # rows stay together, columns inside a row are shuffled
    r, c, v = r[perm][order], c[perm][order], v[perm][order]
    indptr = np.r_[0, np.cumsum(np.bincount(r, minlength=X.shape[0]))]
    out = sp.csr_matrix((v, c, indptr), shape=X.shape)
    assert not out.has_canonical_format
    return out


def _rel_weight_diff(a, b):
    return float(np.abs(a.weights_ - b.weights_).max() / np.abs(b.weights_).max())


CASES = [("digits", dict(n_iter=80, max_neurons=60, random_state=0)),
         ("topics", dict(n_iter=40, max_neurons=40, random_state=0))]


@pytest.mark.parametrize("dtype,gate", [(np.float64, 1e-12), (np.float32, 1e-6)])
@pytest.mark.parametrize("data,kw", CASES)
def test_fit_on_csr_equals_fit_on_dense(data, kw, dtype, gate):
    """Same lattice, labels / predictions and n_iter_; weights differ only through the moments (float64 from the
    stored entries against NumPy's in X's dtype).  Largest weight difference over largest weight, measured with
    this file's inputs on the CPU stand-in (gates: 1e-12 float64, 1e-6 float32):
      float64: digits VQ 7.0e-16, classifier 7.0e-16, entropy 1.1e-15, weighted VQ 5.8e-16;
               topics VQ 9.1e-17, classifier 9.1e-17, entropy 1.2e-16, weighted VQ 1.1e-16
      float32: digits VQ 1.2e-8, classifier 1.2e-8, entropy 3.4e-8, weighted VQ 4.6e-16;
               topics VQ 2.3e-8, classifier 2.3e-8, entropy 2.3e-8, weighted VQ 1.5e-16
    (a weighted fit takes its moments in float64 on both sides, whatever the dtype of X: only their order of
    summation differs).  Neurons / n_iter_: digits 25 / 52 (entropy 56 / 79, weighted 43 / 65), topics 35 / 39
    (entropy 36, weighted 41)."""
    Xs, y = digits_csr(dtype) if data == "digits" else topics(dtype=dtype)
    Xd = Xs.toarray()
    w = np.random.default_rng(7).integers(0, 4, Xs.shape[0])
    fits = [("VQ", SomVQ, {}, False, None), ("classifier", SomClassifier, {}, True, None),
            ("entropy", SomClassifier, dict(growth_criterion="entropy", spreading_factor=0.4), True, None),
            ("weighted VQ", SomVQ, {}, False, w)]
    for name, cls, extra, supervised, sw in fits:
        fit_kw = {} if sw is None else {"sample_weight": sw}
        a = cls(backend=CsrOracleBackend(), **kw, **extra).fit(Xs, y if supervised else None, **fit_kw)
        b = cls(backend=CsrOracleBackend(), **kw, **extra).fit(Xd, y if supervised else None, **fit_kw)
        diff = _rel_weight_diff(a, b)
        print(f"{data} {np.dtype(dtype).name} {name}: max |dW| / max |W| = {diff:.2e}, neurons {len(a.neurons_)}, "
              f"n_iter {a.n_iter_}")
        assert a.neurons_ == b.neurons_ and a.n_iter_ == b.n_iter_
        assert a.weights_.dtype == b.weights_.dtype
        if supervised:
            assert np.array_equal(a._extract_values_from_graph("label"), b._extract_values_from_graph("label"))
            assert np.array_equal(a.predict(Xs[:200]), b.predict(Xd[:200]))
        else:
            assert np.array_equal(a.labels_, b.labels_)
            assert np.array_equal(a.predict(Xs), b.predict(Xd))
        assert diff <= gate


def test_host_moments_from_the_stored_entries():
    for Xs in (digits_csr()[0], topics(N=1000, d=1000, empty_rows=20, stored_zeros=50, unused_tail=64)[0],
               topics(N=700, d=2048, dtype=np.float32)[0]):
        D = Xs.toarray().astype(np.float64)
        n = D.shape[0]
        want = np.var(D, axis=0) * n
        got = SomVQ._sparse_column_s2(Xs)
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * want.max())
        w = np.random.default_rng(1).integers(0, 4, n)
        Dr = np.repeat(D, w, axis=0)
        want_w = np.var(Dr, axis=0) * Dr.shape[0]
        got_w = SomVQ._sparse_column_s2(Xs, w.astype(np.float64), float(w.sum()))
        np.testing.assert_allclose(got_w, want_w, rtol=1e-12, atol=1e-12 * want_w.max())
    # what the estimator makes of them
    Xs, _ = digits_csr()
    est = SomVQ(random_state=0, backend=CsrOracleBackend())
    X, _ = est._check_input_data(Xs)
    est._engine().load(X)
    est._load_resident(X)
    est._attach_sample_weight(X, None)
    est._initialize_som(X)
    D = Xs.toarray()
    np.testing.assert_allclose(est._total_variance, np.var(D, axis=0).sum(), rtol=1e-12)
    np.testing.assert_allclose(est.growing_threshold_, 150 * -np.log(0.5) * np.linalg.norm(np.std(D, axis=0, ddof=1)),
                               rtol=1e-12)
    assert np.array_equal(est.weights_, np.random.default_rng(0).choice(a=D, size=4, replace=False))


def test_queries_on_csr_equal_the_dense_calls():
    Xs, y = digits_csr()
    Xd = Xs.toarray()
    vq = SomVQ(random_state=0, n_iter=30, backend=CsrOracleBackend()).fit(Xs)
    assert np.array_equal(vq.predict(Xs), vq.predict(Xd))
    assert vq.calculate_quantization_error(Xs) == vq.calculate_quantization_error(Xd)
    assert np.array_equal(vq.transform(Xs), vq.transform(Xd))
    clf = SomClassifier(random_state=0, n_iter=30, backend=CsrOracleBackend()).fit(Xs, y)
    assert np.array_equal(clf.predict_proba(Xs), clf.predict_proba(Xd))
    assert np.array_equal(clf.predict(Xs), clf.predict(Xd))
    assert np.array_equal(clf.transform(Xs[:700]), clf.transform(Xd[:700]))
    # several chunks, the last one short: rows are coded independently, but the host default's BLAS products
    # depend on the batch they are part of -- equal to rounding there (bit for bit on the device:
    # tests/test_gpu_csr.py)
    vq._SPARSE_CODE_ROWS = clf._SPARSE_CODE_ROWS = 500
    np.testing.assert_allclose(vq.transform(Xs[:1300]), vq.transform(Xd[:1300]), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(clf.predict_proba(Xs[:1300]), clf.predict_proba(Xd[:1300]), rtol=1e-10, atol=1e-13)
    with pytest.raises(TypeError):
        vq.topographic_function(Xs)          # dense X only, as before
    # integer sparse data is converted to float64 as dense integer data is
    Xi = sp.csr_matrix(Xd.astype(np.int64))
    assert np.array_equal(vq.predict(Xi), vq.predict(Xd))


def test_vertical_growth_on_csr_takes_the_host_subsets():
    Xs, y = digits_csr()
    Xd = Xs.toarray()
    kw = dict(random_state=0, n_iter=30, max_neurons=12, vertical_growth=True, min_samples_vertical_growth=60)
    a = SomClassifier(backend=CsrOracleBackend(), **kw).fit(Xs, y)
    b = SomClassifier(backend=CsrOracleBackend(), **kw).fit(Xd, y)
    kids_a = [n for n, at in a.som_.nodes.items() if "som" in at]
    kids_b = [n for n, at in b.som_.nodes.items() if "som" in at]
    assert kids_a == kids_b and len(kids_a) >= 1
    for n in kids_a:
        assert a.som_.nodes[n]["som"].neurons_ == b.som_.nodes[n]["som"].neurons_
    np.testing.assert_allclose(a.predict_proba(Xs[:150]), b.predict_proba(Xd[:150]), rtol=1e-9, atol=1e-12)


def test_validation_clone_pickle_and_other_sparse_formats():
    Xs, y = digits_csr()
    with pytest.raises(ValueError, match="sharded_input"):
        SomVQ(random_state=0, n_iter=3, sharded_input=True, backend=CsrOracleBackend()).fit(Xs)
    bad = Xs.copy()
    bad.data[17] = np.nan
    with pytest.raises(ValueError):
        SomVQ(random_state=0, n_iter=3, backend=CsrOracleBackend()).fit(bad)
    bad.data[17] = np.inf
    with pytest.raises(ValueError):
        SomClassifier(random_state=0, n_iter=3, backend=CsrOracleBackend()).fit(bad, y)
    est = SomVQ(random_state=0, n_iter=12, backend=CsrOracleBackend()).fit(Xs)
    twin = clone(est).fit(Xs)
    assert twin.neurons_ == est.neurons_ and np.array_equal(twin.weights_, est.weights_)
    back = pickle.loads(pickle.dumps(est))
    back.backend = CsrOracleBackend()
    assert np.array_equal(back.predict(Xs), est.predict(Xs))
    for other in (Xs.tocsc(), Xs.tocoo(), uncanonical(Xs)):     # converted / made canonical, not refused
        e2 = SomVQ(random_state=0, n_iter=12, backend=CsrOracleBackend()).fit(other)
        assert e2.neurons_ == est.neurons_
        np.testing.assert_allclose(e2.weights_, est.weights_, rtol=1e-12, atol=1e-12)
        assert np.array_equal(e2.predict(other), est.labels_)


def test_canonical_csr_leaves_the_callers_matrix_alone():
    from dbgsom_amd.backend import canonical_csr

    Xs, _ = topics(N=300, d=1000, dtype=np.float32, empty_rows=7, stored_zeros=11)
    messy = uncanonical(Xs)
    before = (messy.indptr.copy(), messy.indices.copy(), messy.data.copy())
    csr, indptr, indices, data = canonical_csr(messy)
    assert all(np.array_equal(a, b) for a, b in zip(before, (messy.indptr, messy.indices, messy.data)))
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert np.array_equal(csr.toarray(), Xs.toarray())          # halves add up exactly
    lib = _native.load()
    assert lib.dbgsom_csr_check(indptr.ctypes.data, indices.ctypes.data, csr.shape[0], csr.shape[1], data.size) == 0
    _, _, _, d64 = canonical_csr(sp.csr_matrix(Xs.toarray().astype(np.int32)))
    assert d64.dtype == np.float64


def test_csr_check_reports_faults_as_status_codes():
    lib = _native.load()

    def check(indptr, indices, N, d):
        indptr = np.asarray(indptr, dtype=np.int64)
        indices = np.asarray(indices, dtype=np.int32)
        rc = lib.dbgsom_csr_check(indptr.ctypes.data, indices.ctypes.data, N, d, indices.size)
        return rc, lib.dbgsom_last_error()

    assert check([0, 2, 3], [0, 4, 1], 2, 5)[0] == 0
    assert check([0, 0, 0], [], 2, 5)[0] == 0                                  # empty rows
    rc, msg = check([0, 2, 1, 3], [0, 1, 2], 3, 5)
    assert rc == -1 and b"not monotone" in msg
    rc, msg = check([0, 2, 3], [0, 5, 1], 2, 5)
    assert rc == -1 and b"out of range" in msg
    rc, msg = check([0, 2, 3], [4, 1, 1], 2, 5)
    assert rc == -1 and b"not strictly ascending" in msg
    rc, msg = check([0, 2, 3], [1, 1, 1], 2, 5)                                # a duplicate is not ascending either
    assert rc == -1 and b"not strictly ascending" in msg
    rc, msg = check([1, 2, 3], [0, 1, 2], 2, 5)
    assert rc == -1 and b"indptr[0]" in msg
    rc, msg = check([0, 1, 2], [0, 1, 2], 2, 5)
    assert rc == -1 and b"indptr[N]" in msg
    with pytest.raises(ValueError, match="not monotone"):
        _native.call("dbgsom_csr_check", np.array([0, 2, 1], dtype=np.int64).ctypes.data,
                     np.array([0, 1], dtype=np.int32).ctypes.data, 2, 5, 1)
