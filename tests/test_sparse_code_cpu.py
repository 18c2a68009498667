"""CPU: the sparse-coding ABI rejects bad arguments with status codes (before any device work), and
the host default of HotPathBackend.sparse_code is scikit-learn's SparseCoder."""
import ctypes
import warnings

import numpy as np

from dbgsom_amd import _native
from dbgsom_amd.backend import HotPathBackend


def _err():
    return _native.load().dbgsom_last_error()


def test_sparse_code_argument_errors_are_status_codes():
    lib = _native.load()
    cnt = (ctypes.c_uint64 * len(_native.SC_COUNTS))()
    # x_dtype bfloat16 is not a query dtype
    rc = lib.dbgsom_sparse_code(None, _native.BF16, 10, 4, 4, None, 5, 4, 1000, 0, None, 0, None, None, cnt,
                                None, 0, None)
    assert rc == -1 and b"x_dtype" in _err()
    rc = lib.dbgsom_sparse_code(None, _native.F64, 10, 4, 3, None, 5, 4, 1000, 0, None, 0, None, None, cnt,
                                None, 0, None)
    assert rc == -1 and b"bad shape" in _err()
    rc = lib.dbgsom_sparse_code(None, _native.F64, 10, 4, 4, None, 5, 4, -1, 0, None, 0, None, None, cnt,
                                None, 0, None)
    assert rc == -1 and b"max_iter" in _err()
    rc = lib.dbgsom_sparse_code(None, _native.F64, 10, 4, 4, None, 5, 4, 1000, 0, None, 0, None, None, cnt,
                                None, 0, None)
    assert rc == -1 and b"null pointer" in _err()
    buf = (ctypes.c_double * 64)()
    rc = lib.dbgsom_sparse_code(buf, _native.F64, 2, 4, 4, buf, 5, 4, 1000, 0, None, 0, None, buf, cnt,
                                None, 0, None)
    assert rc == -1 and b"proba needs P" in _err()
    rc = lib.dbgsom_sparse_code(buf, _native.F64, 2, 4, 4, buf, 5, 4, 1000, 0, None, 0, buf, None, cnt,
                                None, 0, None)
    assert rc == -1 and b"workspace" in _err()
    assert lib.dbgsom_sparse_code_workspace_bytes(-1, 4, 5, 1000) == 0
    assert lib.dbgsom_sparse_code_workspace_bytes(10, 4, 5, 1000) > 10 * 5 * 8
    # the context call: a null context is refused
    assert lib.dbgsom_sparse_code_stage_ms(None) == -1
    assert lib.dbgsom_ctx_sparse_code(None, None, _native.F64, 0, 4, None, 5, 1000, None, 0, None, None, cnt) != 0


def test_host_default_is_sparse_coder():
    from sklearn.decomposition import SparseCoder
    from sklearn.preprocessing import normalize

    rng = np.random.default_rng(3)
    W = rng.normal(size=(40, 12))
    X = rng.normal(size=(60, 12))
    X[5] = 0.0
    be = HotPathBackend()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        code = be.sparse_code(W, X)
        ref = SparseCoder(dictionary=normalize(W), positive_code=True, transform_alpha=0,
                          transform_algorithm="lasso_lars").transform(normalize(X))
        assert np.array_equal(code, ref)
        P = rng.random((40, 3))
        pr = be.sparse_code(W, X, P=P)
    raw = ref @ P
    np.testing.assert_array_equal(pr, raw / raw.sum(axis=1)[:, None])
    assert np.isnan(pr[5]).all()
