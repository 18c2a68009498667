"""MI355X: the CSR kernels of csrc/csr.hip called raw through the CSR section of include/dbgsom_hip.h, at the shapes
the context's inputs never reach -- rows of more stored entries than a workgroup has threads, neuron lists of several
chunks, prototype counts around the 256-prototype blocks of the search, empty groups of rows, matrices without a
stored entry, any d >= 1, transposition in two launches -- against plain references on ``X.toarray()``
(tests/csr_device.py, tests/device_abi.py).  Outputs are pre-filled with NaN (indices with -7).  The chains, the
transposition, the expansion, the integer results and the stable order are compared bit for bit, the per-neuron sums
within (n + 2) u sum |terms| (weighted: 2 n + 4) of np.longdouble sums, and with the dense kernels on the wide
shapes bit for bit."""
import numpy as np
import pytest

from tests import csr_device as cd
from tests import device_abi as da
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu
GUARD = 1024          # elements behind an output that must stay as they were


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


@pytest.fixture(scope="module")
def nat():
    from dbgsom_amd import _native

    _native.load()
    return _native


def _sync():
    import torch

    torch.cuda.synchronize()


def _full(shape, value, dtype):
    import torch

    return torch.full(shape, value, dtype=getattr(torch, dtype), device="cuda")


def _ptr(t):
    """a zero-size tensor has no storage: NULL"""
    return t.data_ptr() if t.numel() else None


class DevCsr:
    """the three arrays of a CSR matrix as plain device tensors"""

    def __init__(self, X):
        indptr, indices, data = cd.arrays(X)
        self.N, self.d = X.shape
        self.code = da.F32 if data.dtype == np.float32 else da.F64
        self.indptr, self.indices, self.data = da.dev(indptr), da.dev(indices), da.dev(data)
        self.ptrs = (self.indptr.data_ptr(), _ptr(self.indices), _ptr(self.data))


def _csr_norms(nat, X):
    """dbgsom_csr_row_sqnorms -> device tensor (the caller synchronises)"""
    out = _full((X.N,), float("nan"), "float64")
    nat.call("dbgsom_csr_row_sqnorms", X.ptrs[0], X.ptrs[2], X.code, X.N, out.data_ptr(), da.stream())
    return out


# ---- 1. dbgsom_csr_row_sqnorms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", cd.NORM_N)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_csr_row_sqnorms_are_the_chain_over_the_stored_entries(nat, o, dtype, N):
    rng = np.random.default_rng(N)
    X = cd.rows_csr(cd.norm_lengths(N, rng), cd.NORM_D, dtype, rng, stored_zeros=5)
    out = _csr_norms(nat, DevCsr(X))
    _sync()
    assert np.array_equal(out.cpu().numpy(), o.row_sqnorms_chain(X.toarray()))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_csr_row_sqnorms_of_a_matrix_without_entries_are_zero(nat, dtype):
    rng = np.random.default_rng(0)
    X = DevCsr(cd.rows_csr(np.zeros(257, dtype=np.int64), 9, dtype, rng))
    assert X.data.numel() == 0 and X.ptrs[2] is None
    out = _csr_norms(nat, X)
    _sync()
    assert (out.cpu().numpy() == 0).all()


# ---- 2. dbgsom_csr_transpose_weights ------------------------------------------------------------------------------
def _transpose(nat, W_t, M, d, ldw, w_ptr=None):
    """-> (Wt with its guard behind, ldwt)"""
    ldwt = nat.load().dbgsom_csr_wt_ld(M)
    Wt = _full((d * ldwt + GUARD,), float("nan"), "float64")
    nat.call("dbgsom_csr_transpose_weights", w_ptr or W_t.data_ptr(), M, d, ldw, Wt.data_ptr(), ldwt, da.stream())
    return Wt, ldwt


@pytest.mark.parametrize("M,d,ldw", cd.TRANSPOSE_SHAPES)
def test_transpose_weights_with_a_row_stride(nat, M, d, ldw):
    W = np.random.default_rng(M + d).normal(size=(M, d))
    W_t, w_ptr = da.stage(W, ldw, 0, "f64")                     # the columns d .. ldw hold NaN
    Wt, ldwt = _transpose(nat, W_t, M, d, ldw, w_ptr)
    _sync()
    assert ldwt == cd.wt_ld(M) and ldwt % cd.CT == 0 and ldwt >= M
    got = Wt.cpu().numpy()
    body = got[:d * ldwt].reshape(d, ldwt)
    assert np.array_equal(body[:, :M], W.T)
    assert (body[:, M:] == 0).all()
    assert np.isnan(got[d * ldwt:]).all()


def test_transpose_weights_in_two_launches(nat):
    """d = 65535 * 32 + 33: the second launch covers one whole tile and a tail of one column.  Wt (4.3 GB) is
    checked where it is."""
    import torch

    M, d = cd.TRANSPOSE_MULTI
    gen = torch.Generator(device="cuda").manual_seed(5)
    W = torch.randn((M, d), dtype=torch.float64, device="cuda", generator=gen)
    Wt, ldwt = _transpose(nat, W, M, d, d)
    _sync()
    body = Wt[:d * ldwt].view(d, ldwt)
    same = bool(torch.equal(body[:, :M], W.t()))
    zeros = bool((body[:, M:] == 0).all())
    guard = bool(torch.isnan(Wt[d * ldwt:]).all())
    # (where a difference is, for the message: the columns of the second launch start at 65535 * 32)
    bad = torch.nonzero((body[:, :M] != W.t()).any(dim=1)).flatten()[:3].tolist() if not same else []
    del body, Wt, W
    torch.cuda.empty_cache()
    assert same, f"first differing columns {bad}"
    assert zeros and guard


# ---- 3. dbgsom_bmu_csr ----------------------------------------------------------------------------------------------
def _bmu_csr_and_dense(nat, o, X, W, k, round_f32):
    """dbgsom_bmu_csr with xx from dbgsom_csr_row_sqnorms, ww from dbgsom_row_sqnorms and Wt from the transposition,
    and dbgsom_bmu on the densified rows with the same xx and ww -> ((dist, idx) CSR, (dist, idx) dense) shaped as
    o.bmu_chain returns them"""
    M, d = W.shape
    dtype = "f32" if X.dtype == np.float32 else "f64"
    D = X.toarray()
    Xc = DevCsr(X)
    xx = _csr_norms(nat, Xc)
    W_t = da.dev(W)
    ww = _full((M,), float("nan"), "float64")
    nat.call("dbgsom_row_sqnorms", W_t.data_ptr(), da.F64, M, d, d, ww.data_ptr(), da.stream())
    Wt, ldwt = _transpose(nat, W_t, M, d, d)
    N = Xc.N
    out = []
    D_t, d_ptr = da.stage(D, d, 0, dtype)
    for sparse in (True, False):
        idx = _full((N, k), -7, "int64")
        dist = _full((N, k), float("nan"), "float64")
        if sparse:
            nat.call("dbgsom_bmu_csr", *Xc.ptrs, Xc.code, N, xx.data_ptr(), Wt.data_ptr(), ldwt, M, ww.data_ptr(), k,
                     round_f32, idx.data_ptr(), dist.data_ptr(), da.stream())
        else:
            nat.call("dbgsom_bmu", d_ptr, Xc.code, N, d, d, xx.data_ptr(), W_t.data_ptr(), M, ww.data_ptr(), k, round_f32,
                     idx.data_ptr(), dist.data_ptr(), da.stream())
        _sync()
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        out.append((dist.reshape(-1), idx.reshape(-1)) if k == 1 else (dist, idx))
    assert np.array_equal(xx.cpu().numpy(), o.row_sqnorms_chain(D))
    assert np.array_equal(ww.cpu().numpy(), o.row_sqnorms_chain(W), equal_nan=True)
    return out[0], out[1], ww.cpu().numpy()


def _check_bmu(nat, o, X, W, k, round_f32=0):
    (dist, idx), (dd, di), ww = _bmu_csr_and_dense(nat, o, X, W, k, round_f32)
    rd, ri = o.bmu_chain(X.toarray(), W.astype(np.float32) if round_f32 else W, k)
    assert np.array_equal(idx, ri)
    assert np.array_equal(dist, rd)
    assert np.array_equal(idx, di) and np.array_equal(dist, dd)          # "dbgsom_bmu for CSR samples"
    if round_f32:
        assert np.array_equal(dist, dist.astype(np.float32).astype(np.float64))
    return dist, idx, ww


@pytest.mark.parametrize("dtype,N,d,M,k,round_f32", cd.BMU_CSR_CASES)
def test_bmu_csr_is_the_chain_and_the_dense_search(nat, o, dtype, N, d, M, k, round_f32):
    X, W = cd.search_case(dtype, N, d, M, k, round_f32)
    dist, idx, _ = _check_bmu(nat, o, X, W, k, round_f32)
    if M >= 33:
        assert (idx != 7).all()                                          # the whole-NaN prototype never wins
    assert not np.isnan(dist).any()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_bmu_csr_of_a_matrix_without_entries(nat, o, dtype):
    """every distance is sqrt(ww_j): the smallest wins, for every row alike"""
    rng = np.random.default_rng(1)
    X = cd.rows_csr(np.zeros(6, dtype=np.int64), 5, dtype, rng)
    assert X.nnz == 0
    W = cd.prototypes(257, 5, rng)
    dist, idx, ww = _check_bmu(nat, o, X, W, 2)
    first = int(np.nanargmin(ww))
    assert (idx[:, 0] == first).all() and (dist[:, 0] == np.sqrt(ww[first])).all()
    rest = np.where(np.arange(ww.size) == first, np.inf, ww)
    assert (idx[:, 1] == int(np.nanargmin(rest))).all() and (dist[:, 1] == np.sqrt(np.nanmin(rest))).all()


def test_bmu_csr_ties_go_to_the_lowest_index_across_blocks(nat, o):
    X, W = cd.tie_case()
    dist, idx, _ = _check_bmu(nat, o, X, W, 2)
    assert (idx[:, 0] < cd.TIE_BASE).all()
    assert (idx[:, 1] > idx[:, 0]).all() and (dist[:, 0] == dist[:, 1]).all()


# ---- 4. dbgsom_csr_densify ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,ld", cd.DENSIFY_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_csr_densify_into_padded_rows(nat, dtype, N, d, ld):
    rng = np.random.default_rng(N + d)
    X = cd.rows_csr(cd.densify_lengths(N, d, rng), d, dtype, rng, stored_zeros=2 if N > 1 else 0)
    Xc = DevCsr(X)
    out = _full((N * ld + GUARD,), float("nan"), "float32" if dtype == "f32" else "float64")
    nat.call("dbgsom_csr_densify", *Xc.ptrs, Xc.code, N, d, ld, out.data_ptr(), da.stream())
    _sync()
    got = out.cpu().numpy()
    body = got[:N * ld].reshape(N, ld)
    assert np.array_equal(body[:, :d], X.toarray())
    assert (body[:, d:] == 0).all()
    assert np.isnan(got[N * ld:]).all()


# ---- 5. dbgsom_accumulate_csr ---------------------------------------------------------------------------------------
def _split(v, M, d):
    return v[:M * d].reshape(M, d), v[M * d:M * d + M], v[M * d + M:M * d + 2 * M], v[M * d + 2 * M:]


def _accumulate_csr_call(nat, case, status=True):
    """-> (the M (d + 3) sums, status word or None, the first N int32 of the workspace), called twice: the second
    call's bits must be the first's"""
    X, winners, kw, dist, M, sw, _ = case
    lib = nat.load()
    Xc = DevCsr(X)
    N, d = Xc.N, Xc.d
    win_t, kw_t, dist_t = da.dev(winners), da.dev(kw), da.dev(dist)
    sw_t = da.dev(sw) if sw is not None else None
    nbytes = lib.dbgsom_accumulate_csr_workspace_bytes(N, d, M)
    assert nbytes > 0
    ws_t, ws = da.workspace(nbytes)
    outs = []
    for _ in range(2):
        sums = _full((M * (d + 3),), float("nan"), "float64")
        st = _full((1,), 77, "int32") if status else None
        nat.call("dbgsom_accumulate_csr", *Xc.ptrs, Xc.code, N, d, win_t.data_ptr(), kw_t.data_ptr(),
                 sw_t.data_ptr() if sw is not None else None, dist_t.data_ptr(), M, sums.data_ptr(),
                 st.data_ptr() if status else None, ws, nbytes, da.stream())
        _sync()
        outs.append((sums.cpu().numpy(), int(st.cpu()[0]) if status else None))
    assert np.array_equal(outs[0][0], outs[1][0], equal_nan=True) and outs[0][1] == outs[1][1]   # the same bits twice
    skip = ws - ws_t.data_ptr()
    order = ws_t[skip:skip + 4 * N].cpu().numpy().view(np.int32)
    return outs[0][0], outs[0][1], order


def _check_accumulate_csr(nat, case, status=True, keep=None):
    X, winners, kw, dist, M, sw, _ = case
    v, st, order = _accumulate_csr_call(nat, case, status)
    cd.check_sums(case, *_split(v, M, X.shape[1]), keep=keep)
    inside = (winners >= 0) & (winners < M)
    if status:
        assert (st != 0) == (not inside.all())
    if inside.all():
        assert np.array_equal(order, np.argsort(winners, kind="stable"))       # the header's contract for order_dev


@pytest.mark.parametrize("weights", [None, "int", "frac"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_accumulate_csr_rows_longer_than_a_workgroup(nat, dtype, weights):
    _check_accumulate_csr(nat, cd.long_rows_case(dtype, weights))


@pytest.mark.parametrize("weights", [None, "frac"])
@pytest.mark.parametrize("d,per_row", cd.LIST_SHAPES)
def test_accumulate_csr_list_lengths_around_the_chunk_size(nat, d, per_row, weights):
    _check_accumulate_csr(nat, cd.list_case(d, per_row, weights))


@pytest.mark.parametrize("M", sorted(da.GROUP_CASES))
@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_csr_second_level_sum(nat, M, weighted):
    _check_accumulate_csr(nat, cd.group_case(M, weighted))


@pytest.mark.parametrize("d", cd.FINALIZE_D)
def test_accumulate_csr_finalize_column_loop_and_one_column(nat, d):
    _check_accumulate_csr(nat, cd.finalize_case(d))


@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_csr_status_and_skipped_rows(nat, weighted):
    for bad in (False, True):              # in range: status 0; one -1 and one M: status set, the two rows skipped
        for status in (True, False):       # (False: status_dev = NULL)
            _check_accumulate_csr(nat, cd.status_case(weighted, bad), status)


@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_csr_of_no_rows_returns_zeros(nat, weighted):
    M, d = 7, 5
    sums = _full((M * (d + 3),), float("nan"), "float64")
    st = _full((1,), 77, "int32")
    ws_t, ws = da.workspace(4096)
    indptr = da.dev(np.zeros(1, dtype=np.int64))
    sw = da.dev(np.zeros(1)) if weighted else None
    nat.call("dbgsom_accumulate_csr", indptr.data_ptr(), None, None, da.F32, 0, d, None, None,
             sw.data_ptr() if weighted else None, None, M, sums.data_ptr(), st.data_ptr(), ws, 4096, da.stream())
    _sync()
    assert (sums.cpu().numpy() == 0).all() and int(st.cpu()[0]) == 0


def test_accumulate_csr_does_not_stream_rows_of_weight_zero(nat):
    """a NaN stored in a row of weight 0 reaches no sum (the reference is built from the other rows: 0 * NaN would
    poison it)"""
    case, keep = cd.zero_weight_nan_case()
    assert np.isnan(case[0].data).any()
    _check_accumulate_csr(nat, case, keep=keep)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype,d", cd.WIDE_SHAPES)
def test_accumulate_csr_equals_the_dense_call_on_wide_rows(nat, dtype, d, weighted):
    """include/dbgsom_hip.h, CSR section: where the dense call adds a column in list order, the same M (d + 3) doubles"""
    assert da.segsum_class(dtype, d, d, 0)[1] == "wide"
    case = cd.wide_case(dtype, d, weighted)
    X, winners, kw, dist, M, sw, _ = case
    got, st, _ = _accumulate_csr_call(nat, case)
    lib = nat.load()
    N = X.shape[0]
    xt, xptr = da.stage(X.toarray(), d, 0, dtype)
    name = "dbgsom_accumulate_weighted" if weighted else "dbgsom_accumulate"
    nbytes = getattr(lib, name + "_workspace_bytes")(N, d, M)
    ws_t, ws = da.workspace(nbytes)
    win_t, kw_t, dist_t = da.dev(winners), da.dev(kw), da.dev(dist)
    sw_t = da.dev(sw) if weighted else None
    sums = _full((M * (d + 3),), float("nan"), "float64")
    args = [xptr, da.CODE[dtype], N, d, d, win_t.data_ptr(), kw_t.data_ptr()] + ([sw_t.data_ptr()] if weighted else [])
    nat.call(name, *args, dist_t.data_ptr(), M, sums.data_ptr(), None, ws, nbytes, da.stream())
    _sync()
    dense = sums.cpu().numpy()
    assert st == 0 and not np.isnan(dense).any()
    assert np.array_equal(got, dense)
    S, K, a, E = _split(got, M, d)
    n = np.bincount(winners, minlength=M)
    assert np.array_equal(a, n if sw is None else np.bincount(winners, weights=sw, minlength=M))
    assert (S[n == 0] == 0).all() and np.abs(S[n > 0]).max() > 0


# ---- 6. through the context -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_context_on_long_rows_equals_the_dense_backend(o, dtype):
    """rows of 600 .. 800 stored entries (some empty, some full) at d = 2048, M = 4: lists of about 375 rows, three
    chunks each"""
    from tests.test_gpu_csr import _pair, _prototypes, _same_epoch

    rng = np.random.default_rng(8)
    X = cd.rows_csr(cd.context_lengths(rng), cd.CTX_D, dtype, rng, stored_zeros=200)
    D = X.toarray()
    M = cd.CTX_M
    W = _prototypes(X, M)
    hop = gi.lattice_hops(2, 2)
    gamma = 1.0 / float(np.var(D.astype(np.float64), axis=0).sum())
    cs, dn = _pair(X)
    other = type(cs)(0)
    other.csr_densify_below = 0
    want_d, want_i = o.bmu_chain(D, W, 2)
    for what, (dist, idx) in (("resident", cs.bmu(W, 2)), ("query", other.bmu(W, 2, X=X))):
        assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d), what
    other.release()
    kw = np.random.default_rng(2).random(X.shape[0])
    sw = np.random.default_rng(7).integers(0, 4, X.shape[0]).astype(np.float64)
    assert (sw == 0).any()
    for weights in (None, sw):
        for be in (cs, dn):
            be.set_sample_weight(weights)
        ra, rb = cs.epoch(W, hop, 1.4, gamma, "compact", True), dn.epoch(W, hop, 1.4, gamma, "compact", True)
        _same_epoch(ra, rb)
        assert np.array_equal(cs.read_sums(M), dn.read_sums(M))
        n = np.bincount(ra.winners, minlength=M)
        assert n.max() > 2 * cd.CCH                                       # a list of three chunks at least
        ua = cs.update(W, hop, 1.4, kw, ra.winners, ra.distances, "aligned")
        ub = dn.update(W, hop, 1.4, kw, rb.winners, rb.distances, "aligned")
        for p, q in zip(ua, ub):
            assert np.array_equal(p, q)
        assert np.array_equal(cs.read_sums(M), dn.read_sums(M))
    cs.release()
    dn.release()
