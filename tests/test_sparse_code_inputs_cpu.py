"""CPU: the planted inputs of tests/sparse_code_inputs.py meet, by scikit-learn alone, the conditions that
tests/test_gpu_sparse_code_paths.py relies on: no ConvergenceWarning, final supports in the range that
sends a row to the intended pass, iteration counts that do not depend on the order of the features, and
codes that move under a feature permutation by at most 1/100 of the parity gate (1e-12 for float64
queries, 1e-8 for float32).  A case that misses a condition gets another seed or shape in
sparse_code_inputs.py, never a looser bound here."""
import warnings

import numpy as np
import pytest

from tests import sparse_code_inputs as si

DTYPES = ("float64", "float32")


def _conditions(W, X, max_iter=1000):
    """Reference on (W, X) and on the feature-permuted problem; returns (codes, iterations, support sizes)
    after asserting that no warning is raised, the iteration counts agree and the codes are within the
    self-noise bound of the query dtype."""
    code, iters = si.reference(W, X, max_iter)        # (a warning is an error in there)
    Wp, Xp = si.permuted(W, X)
    assert Xp.dtype == X.dtype
    code_p, iters_p = si.reference(Wp, Xp, max_iter)
    assert np.array_equal(iters, iters_p), "iteration counts depend on the feature order"
    moved = np.abs(code - code_p).max() if code.size else 0.0
    print("self-noise %.3e (%s)" % (moved, X.dtype))
    assert moved <= si.SELF_NOISE[X.dtype], "scikit-learn moves by %.3e against itself" % moved
    return code, iters, np.count_nonzero(code, axis=1)


def test_reference_is_sparse_coder():
    """The row-level reference gives SparseCoder's arrays (and its iteration counts on top)."""
    from sklearn.decomposition import SparseCoder

    W, _, _ = si.case("wide")
    for dtype in DTYPES:
        X, _ = si.case_queries("wide", dtype)
        assert X.dtype == np.dtype(dtype)
        coder = SparseCoder(dictionary=si.normalize(W), positive_code=True, transform_alpha=0,
                            transform_algorithm="lasso_lars")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ref = coder.transform(si.normalize(X))
        code, iters = si.reference(W, X)
        assert np.array_equal(code, ref)
        assert iters.shape == (X.shape[0],) and (iters >= np.count_nonzero(code, axis=1)).all()


def test_planted_needs_noise_and_f32_norms_are_exact():
    with pytest.raises(ValueError):
        si.planted(8, 4, 2, 1, 0.0, 0)
    W, X, _ = si.case("pass1")
    Q = si.f32_queries(X)
    assert Q.dtype == np.float32 and np.abs(Q - X).max() <= np.abs(X).max() * np.sqrt(X.shape[1]) / 4095.0
    _, Qp = si.permuted(W, Q)
    # the float32 normalisation does not depend on the order of the features
    p = np.random.default_rng(12345).permutation(W.shape[1])
    assert np.array_equal(si.normalize(Q)[:, p], si.normalize(Qp))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(si.CASES))
def test_case_meets_its_conditions(name, dtype):
    W, _, _ = si.case(name)
    X, kind = si.case_queries(name, dtype)
    code, iters, support = _conditions(W, X)
    assert iters.max() < 1000, "the max_iter stop must not fire in the default call"
    for s in np.unique(kind):
        lo, hi = si.support_range(name, s)
        sup = support[kind == s]
        print("%s s=%d: support %d..%d, iterations %d..%d" % (name, s, sup.min(), sup.max(),
                                                             iters[kind == s].min(), iters[kind == s].max()))
        assert lo <= sup.min() and sup.max() <= hi
    # (iterations - support) // 2 is the number of drops of a row that skips no degenerate regressor
    drops = (iters - support) // 2
    assert (drops >= 0).all()
    print("%s: %d drops in %d rows" % (name, drops.sum(), X.shape[0]))
    if name in ("pass1", "pass2", "pass2_big"):
        assert (drops[kind != 5] > 0).all()
    if name == "pass2":
        # the short rows never drop: their active set never exceeds the final support, so they stay on the
        # LDS path and the overflow counter is exactly the number of the other rows
        assert np.array_equal(iters[kind == 5], support[kind == 5])
        assert set(np.unique(kind)) == {5, 60, 250}
    if name == "wide":
        assert W.shape[0] > W.shape[1] and support.max() < W.shape[1] * 3 // 4


def test_pass1_active_set_never_outgrows_the_first_pass():
    """`64 < max_active <= 192` on the device needs the peak of the active set, not only its final size:
    taken from the reference's coefficient path."""
    from sklearn.linear_model import lars_path_gram

    W, _, _ = si.case("pass1")
    for dtype in DTYPES:
        X, _ = si.case_queries("pass1", dtype)
        Wn, Xn = si.normalize(W), si.normalize(X)
        gram, cov = np.dot(Wn, Wn.T), np.dot(Wn, Xn.T)
        peak = 0
        for i in range(X.shape[0]):
            _, _, path = lars_path_gram(Xy=cov[:, i], Gram=gram, n_samples=W.shape[1], method="lasso", positive=True,
                                        alpha_min=0, max_iter=1000, return_path=True)
            peak = max(peak, int(np.count_nonzero(path, axis=0).max()))
        print("pass1 %s: largest active set on the path %d" % (dtype, peak))
        assert si.SC_CAP < peak <= si.SC_CAP1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("max_iter", si.MAX_ITERS)
def test_max_iter_cases(max_iter, dtype):
    W, _, _ = si.case("pass1")
    X, _ = si.case_queries("pass1", dtype)
    code, iters, support = _conditions(W, X[:si.MAX_ITER_ROWS], max_iter)
    assert iters.max() == max_iter          # the stop fires
    assert support.max() <= max_iter        # hence slot_cap = min(M, max_iter) suffices
    if max_iter == 0:
        assert not code.any()


def test_sweep_covers_every_axis_value_and_the_corners():
    shapes = si.sweep_shapes()
    assert 35 <= len(shapes) <= 50 and len(set(shapes)) == len(shapes)
    for axis, values in enumerate((si.SWEEP_NQ, si.SWEEP_M, si.SWEEP_D)):
        assert {t[axis] for t in shapes} == set(values)
    for nq in (si.SWEEP_NQ[0], si.SWEEP_NQ[-1]):
        for m in (si.SWEEP_M[0], si.SWEEP_M[-1]):
            for d in (si.SWEEP_D[0], si.SWEEP_D[-1]):
                assert (nq, m, d) in shapes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", si.sweep_shapes(), ids=lambda t: "x".join(map(str, t)))
def test_sweep_case_meets_its_conditions(shape, dtype):
    W, X = si.sweep_case(*shape)
    assert X.shape == (shape[0], shape[2]) and W.shape == (shape[1], shape[2])
    _, _, support = _conditions(W, si.queries(X, dtype))
    assert support.max() <= si.SC_CAP
