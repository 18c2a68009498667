"""MI355X: the covariance pass of csrc/covariance.hip called raw over the shape table of tests/linear_init.py (float32 and
float64 rows; ld > d with NaN in the padding, a base 16 bytes into the allocation, a workspace of 0xFF bytes, sentinels
around the outputs) against the np.longdouble reference within the bound that holds for any summation order; the context
call on host-loaded, borrowed and pad-copied rows; and init="pca" through the estimator."""
import ctypes

import numpy as np
import pytest

from tests import device_abi as da
from tests import linear_init as li

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 8


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


def _guarded(n):
    import torch

    return torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")


def _unguard(t, n):
    h = t.cpu().numpy()
    assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + n:] == SENTINEL), "a store outside the output"
    return h[GUARD:GUARD + n].copy()


def _apply(nat, X, dtype, mean, V, ld, off, ws_bytes=None, mean_null=False):
    """dbgsom_covariance_apply on the staged rows of X -> (status, Z (d, p), colsum (d,))"""
    import torch

    N, d = X.shape
    p = V.shape[1]
    xt, xptr = da.stage(X, ld, off, dtype)
    need = nat.load().dbgsom_covariance_apply_workspace_bytes(N, d, p)
    ws = torch.full((max(need, 1) + 256,), 255, dtype=torch.uint8, device="cuda")
    wptr = (ws.data_ptr() + 255) // 256 * 256
    Vd, md = da.dev(np.array(V)), da.dev(np.array(mean))
    Zt, st = _guarded(d * p), _guarded(d)
    rc = nat.load().dbgsom_covariance_apply(
        ctypes.c_void_p(xptr), da.CODE[dtype], N, d, ld, None if mean_null else ctypes.c_void_p(md.data_ptr()),
        ctypes.c_void_p(Vd.data_ptr()), p, ctypes.c_void_p(Zt.data_ptr() + 8 * GUARD),
        ctypes.c_void_p(st.data_ptr() + 8 * GUARD), ctypes.c_void_p(wptr), need if ws_bytes is None else ws_bytes,
        da.stream())
    torch.cuda.synchronize()
    return rc, _unguard(Zt, d * p).reshape(d, p), _unguard(st, d)


# ---- 1. the raw call over the table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,p,mean_kind", li.SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_covariance_apply_within_the_bound_of_the_exact_pass(nat, dtype, N, d, p, mean_kind):
    X, mean, V, Z, s, zb, sb = li.raw_case(N, d, p, mean_kind, dtype)
    rc, got_Z, got_s = _apply(nat, X, dtype, mean, V, ld=d + 3, off=16 // da.ITEM[dtype])
    assert rc == 0, nat.load().dbgsom_last_error()
    okz, wz = li.within(got_Z, Z, zb)
    oks, ws = li.within(got_s, s, sb)
    print(f"worst |err| / bound: Z {wz:.3g}, colsum {ws:.3g}")
    assert okz and oks


# ---- 2. further raw checks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,p,dtype", [(997, 65, 8, "f32"), (130, 513, 2, "f64"), (129, 1025, 8, "f32")])
def test_same_bits_whatever_the_run_the_stride_and_the_alignment(nat, N, d, p, dtype):
    X, mean, V = li.raw_case(N, d, p, "true", dtype)[:3]
    a = _apply(nat, X, dtype, mean, V, ld=d, off=0)
    b = _apply(nat, X, dtype, mean, V, ld=d, off=0)
    c = _apply(nat, X, dtype, mean, V, ld=d + 5, off=1)
    assert a[0] == b[0] == c[0] == 0
    for x, y in ((a, b), (a, c)):
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
    # mean = NULL is mean = zeros
    z = _apply(nat, X, dtype, np.zeros(d), V, ld=d, off=0)
    n = _apply(nat, X, dtype, np.zeros(d), V, ld=d, off=0, mean_null=True)
    assert np.array_equal(z[1], n[1]) and np.array_equal(z[2], n[2])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nan_or_an_infinity_in_a_row_goes_into_z(nat, bad):
    X, mean, V = li.raw_case(997, 65, 2, "zeros", "f32")[:3]
    X = X.copy()
    X[500, 17] = bad
    rc, Z, s = _apply(nat, X, "f32", mean, V, ld=68, off=0)
    assert rc == 0
    assert not np.isfinite(Z[17]).any() and not np.isfinite(s[17])
    assert np.isfinite(np.delete(s, 17)).all()


def test_a_short_workspace_is_a_status_code(nat):
    X, mean, V = li.raw_case(997, 65, 2, "zeros", "f32")[:3]
    need = nat.load().dbgsom_covariance_apply_workspace_bytes(997, 65, 2)
    rc, Z, s = _apply(nat, X, "f32", mean, V, ld=65, off=0, ws_bytes=need - 1)
    assert rc == -3 and b"workspace too small" in nat.load().dbgsom_last_error()
    assert np.all(Z == SENTINEL) and np.all(s == SENTINEL)           # nothing was launched


# ---- 3. the context call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(64, np.float32), (37, np.float64)])
def test_context_call_on_host_loaded_borrowed_and_pad_copied_rows(d, dtype):
    import torch

    from dbgsom_amd.backend import HipBackend

    N, p = 3000, 8
    X = li.planted(N, d, seed=d, dtype=dtype)
    rng = np.random.default_rng(0)
    V = np.linalg.qr(rng.normal(size=(d, p)))[0]
    mean = np.asarray(X, dtype=np.float64).mean(axis=0)
    wide = torch.full((N, d + 6), float("nan"), dtype=torch.from_numpy(X).dtype, device="cuda")
    wide[:, :d] = torch.from_numpy(X).cuda()
    forms = {"host": lambda be: be.load(X), "tensor": lambda be: be.load_device(torch.from_numpy(X).cuda()),
             "strided tensor": lambda be: be.load_device(wide[:, :d])}
    got = {}
    for name, load in forms.items():
        be = HipBackend(0)
        load(be)
        before = be.sample_traffic()
        got[name] = be.covariance_apply(mean, V)
        after = be.sample_traffic()
        assert after["x_upload_bytes"] - before["x_upload_bytes"] == (d * p + d) * 8, name
        assert after["x_download_bytes"] - before["x_download_bytes"] == (d * p + d) * 8, name
        be.release()
    for name in ("tensor", "strided tensor"):
        assert np.array_equal(got[name][0], got["host"][0]) and np.array_equal(got[name][1], got["host"][1]), name
    Z, s, zb, sb = li.exact(X, mean, V)
    assert li.within(got["host"][0], Z, zb)[0] and li.within(got["host"][1], s, sb)[0]


def test_context_call_refuses_what_it_cannot_do():
    import scipy.sparse

    from dbgsom_amd.backend import HipBackend

    X = li.planted(200, 16, seed=2, dtype=np.float32)
    V, mean = np.eye(16)[:, :2].copy(), np.zeros(16)
    be = HipBackend(0)
    with pytest.raises(RuntimeError, match="load"):
        be.covariance_apply(mean, V)
    be.csr_densify_below = 0
    be.load(scipy.sparse.csr_matrix(X))
    with pytest.raises(ValueError, match="CSR residents"):
        be.covariance_apply(mean, V)
    be.load(X, storage="bf16")
    with pytest.raises(ValueError, match="bfloat16 storage"):
        be.covariance_apply(mean, V)
    be.load(X, incomplete=True)
    with pytest.raises(ValueError, match="missing entries"):
        be.covariance_apply(mean, V)
    be.load(X)
    be.set_sample_weight(np.ones(200))
    with pytest.raises(ValueError, match="sample weights are attached"):
        be.covariance_apply(mean, V)
    be.set_sample_weight(None)
    with pytest.raises(ValueError, match="V must be"):
        be.covariance_apply(mean, np.zeros((16, 9)))
    assert be.covariance_apply(mean, V)[0].shape == (16, 2)
    be.release()


# ---- 4. the estimator -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    """One data set, the fits every estimator test reads: host float32 rows twice, the same rows as a tensor."""
    import torch

    from dbgsom_amd import SomVQ

    X = li.planted(2000, 37, seed=5, dtype=np.float32)
    kw = dict(init="pca", initial_shape=(6, 4), max_neurons=24, n_iter=15)
    starts = []

    def fit(data, **extra):
        est = SomVQ(**kw, **extra)
        orig = est._start_prototypes

        def spy(d):
            out = orig(d)
            starts.append((list(out[0]), np.array(out[1])))
            return out

        est._start_prototypes = spy
        return est.fit(data)

    a, b = fit(X, random_state=0), fit(X, random_state=9)
    t = fit(torch.from_numpy(X).cuda(), random_state=0)
    return X, kw, (a, b, t), starts


def test_principal_directions_against_eigh(fits):
    X, _, (a, _, _), _ = fits
    lam, E = li.reference_spectrum(X)
    print(f"passes {a.init_n_passes_}")
    assert 1 <= a.init_n_passes_ < 60
    np.testing.assert_allclose(a.init_variances_, lam[:2], rtol=1e-12)
    np.testing.assert_allclose(a.init_mean_, np.asarray(X, dtype=np.float64).mean(axis=0), rtol=1e-13)
    for j in range(2):
        err, tol = np.linalg.norm(a.init_directions_[j] - E[j]), li.direction_tolerance(lam, j)
        print(f"direction {j}: |u - e| = {err:.3g}, tolerance {tol:.3g}")
        assert err <= tol


def test_fixed_grid_keeps_its_units_and_fits_repeat_bit_for_bit(fits):
    _, _, (a, b, t), starts = fits
    assert len(a.neurons_) == 24 and a.neurons_ == [(r, c) for r in range(6) for c in range(4)]
    assert a.weights_.shape == (24, 37) and starts[0][1].dtype == np.float64
    for other in (b, t):                       # another seed; the rows as a tensor
        assert np.array_equal(a.init_mean_, other.init_mean_) and np.array_equal(a.init_directions_, other.init_directions_)
        assert np.array_equal(a.init_variances_, other.init_variances_) and a.init_n_passes_ == other.init_n_passes_
        assert np.array_equal(a.weights_, other.weights_) and a.neurons_ == other.neurons_
        assert a.quantization_error_ == other.quantization_error_ and a.n_iter_ == other.n_iter_
    assert all(np.array_equal(starts[0][1], s[1]) and starts[0][0] == s[0] for s in starts[1:])
    assert np.array_equal(a.labels_, b.labels_)


def test_whole_fit_equals_the_stand_in_fit_from_the_same_start(fits):
    """The gates of tests/test_gpu_estimator.py's whole-fit comparisons."""
    from dbgsom_amd import SomVQ
    from oracle.som_oracle import OracleBackend

    X, kw, (a, _, _), starts = fits
    ref = SomVQ(backend=OracleBackend(), random_state=0, **{k: v for k, v in kw.items() if k not in ("init", "initial_shape")})
    ref._start_prototypes = lambda data: (starts[0][0], starts[0][1].copy())
    ref.fit(X)
    assert a.n_iter_ == ref.n_iter_ and a.neurons_ == ref.neurons_
    np.testing.assert_allclose(a.weights_, ref.weights_, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(a.quantization_error_, ref.quantization_error_, rtol=1e-10)
    assert a.topographic_error_ == ref.topographic_error_
    assert np.array_equal(a.labels_, ref.labels_)
