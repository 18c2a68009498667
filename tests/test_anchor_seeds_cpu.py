"""CPU companion of tests/test_gpu_anchor_seed_device.py (tests/anchor_seeds.py holds the tables and references):
the chain of csrc/anchor_chain.h against its NumPy restatement, the references alone inside every cap the GPU file
applies, the tables pairwise as claimed, and the argument errors of the new entry points as status codes before any
HIP call."""
import itertools
import os

import numpy as np
import pytest

from tests import anchor_seeds as an
from tests import device_abi as da


@pytest.fixture(scope="module")
def lib():
    from dbgsom_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.load()


# ---- the chain ------------------------------------------------------------------------------------------------------
def test_header_is_host_only():
    text = open(os.path.join(an.ROOT, "dbgsom_amd", "csrc", "anchor_chain.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>", "<vector>"]
    for word in ("hipStream_t", "hipError_t", "DevBuf", "dbgsom_ctx", "hip_runtime", "__global__"):
        assert word not in text, word


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    """every (input, A, d) of the table through tests/anchor_chain_check.cpp in one run; N = 7 A + 3 rows behind the
    anchors, and once N = A"""
    keys = [(name, A, d) for name in an.CHAIN_INPUTS for A in an.CHAIN_A for d in an.CHAIN_D]
    inputs = {k: an.chain_input(*k) for k in keys}
    cases = [(7 * k[1] + 3, inputs[k][0]) for k in keys] + [(k[1], inputs[k][0]) for k in keys[:3]]
    got = an.run_chain_check(cases, tmp_path_factory.mktemp("chain"))
    return keys, inputs, cases, got


def test_chain_equals_the_numpy_chain(chains):
    keys, inputs, cases, got = chains
    assert {k[1] for k in keys} == {3, 16, 256} and {k[2] for k in keys} == {16, 320}
    for k, (N, rows), (got_rows, got_chain) in zip(keys + keys[:3], cases, got):
        A = rows.shape[0]
        assert np.array_equal(got_rows, an.anchor_rows(N, A)) and np.array_equal(got_rows, [j * N // A for j in range(A)])
        assert got_rows[0] == 0 and (np.diff(got_rows) >= 1).all() and got_rows[-1] < N
        assert got_chain[0] == 0 and np.array_equal(np.sort(got_chain), np.arange(A)), "not a permutation from row 0"
        assert np.array_equal(got_chain, an.chain(rows)), k


def test_chain_ties_go_to_the_lower_row_and_known_answers(chains):
    keys, inputs, _, got = chains
    lower_first = 0
    for k, (_, got_chain) in zip(keys, got):
        X, known = inputs[k]
        name, A, d = k
        if known is not None:
            assert np.array_equal(got_chain, known), k
        if name == "collinear":
            assert np.array_equal(an.chain(X), known)
            lower_first += int(X[known[-1], 0] < 0)       # the row at -3 lost the tie and comes last
        if name == "duplicates":
            # a copy of the current row is at distance 0: the chain takes the copies of a row one after the other, in
            # rising row order
            _, inv = np.unique(X, axis=0, return_inverse=True)
            inv = inv.reshape(-1)[got_chain]
            runs = np.flatnonzero(np.diff(inv) != 0) + 1
            assert len(runs) + 1 == len(np.unique(inv)), "the copies of a row are not consecutive"
            for part in np.split(got_chain, runs):
                assert (np.diff(part) > 0).all(), "copies of a row out of row order"
    # the tie at the start of the collinear chain is met from both sides over the table
    assert lower_first == len(an.CHAIN_A) == len(an.CHAIN_A) * len(an.CHAIN_D) - lower_first


def test_chain_check_rejects_nothing_silently(tmp_path):
    X = np.arange(12, dtype=np.float64).reshape(4, 3)
    (rows, chain), = an.run_chain_check([(9, X)], tmp_path)
    assert rows.tolist() == [0, 2, 4, 6] and chain.tolist() == [0, 1, 2, 3]


# ---- the tables -------------------------------------------------------------------------------------------------------
def test_seed_cases_are_pairwise():
    dims = [an.SEED_A, an.SEED_M, an.SEED_D, an.SEED_KINDS, an.SEED_DTYPES, an.SEED_BUCKETS]
    assert all(len(c) == len(dims) and all(v in dim for v, dim in zip(c, dims)) for c in an.SEED_CASES)
    assert len(set(an.SEED_CASES)) == len(an.SEED_CASES) <= 64
    assert all(c[2] == 16 for c in an.SEED_CASES if c[1] == 8192)
    for a, b in itertools.combinations(range(len(dims)), 2):
        want = set(itertools.product(dims[a], dims[b]))
        if (a, b) == (1, 2):
            want -= {(8192, d) for d in an.SEED_D if d != 16}
        assert {(c[a], c[b]) for c in an.SEED_CASES} == want, (a, b)
    assert an.SEED_A == (1, 15, 16, 17, 255, 256) and an.SEED_M == (1, 15, 16, 17, 63, 64, 65, 130, 1985, 8192)
    assert an.SEED_D == (16, 48, 64, 320)
    assert [r[0] for r in an.SEED_ROWS].count(129) == 1 and all(r[0] in (129, 300) for r in an.SEED_ROWS)
    assert sum(bool(r[1] & an.PRUNE_RETRY) for r in an.SEED_ROWS) == 1 and all(r[1] & an.PRUNE for r in an.SEED_ROWS)
    # the reduction of the last workgroup strides only beyond 16 blocks of 64 prototypes
    assert {M for M in an.SEED_M if (M + 63) // 64 > 16} == {1985, 8192}


def test_tie_sets_sit_where_they_claim():
    where = lambda j: (j // 64, (j % 64) // 16, (j % 16) // 4, j % 4)          # block, wavefront, slot, lane group
    sets = {c[2]: c for c in an.TIE_SETS}
    b = [where(j) for j in (70, 134)]
    assert b[0][0] != b[1][0] and b[0][1:] == b[1][1:]
    w = [where(j) for j in (70, 86)]
    assert w[0][0] == w[1][0] and w[0][1] != w[1][1] and w[0][2:] == w[1][2:]
    s = [where(j) for j in (70, 74)]
    assert s[0][:2] == s[1][:2] and s[0][2] != s[1][2] and s[0][3] == s[1][3]
    q = [where(j) for j in (70, 71)]
    assert q[0][:3] == q[1][:3] and q[0][3] != q[1][3]
    for copies in ((70, 134), (70, 86), (70, 74), (70, 71)):
        assert copies in sets
    # M = 1985: 32 blocks; blocks p and p + 16 are the same thread's, in two rounds
    assert (70 // 64) % 16 == (1094 // 64) % 16 and 70 // 64 < 16 <= 1094 // 64
    assert all(j // 64 >= 16 for j in (1100, 1900)) and 1023 // 64 == 15 and 1024 // 64 == 16 and 1984 == 1985 - 1
    for M, d, copies in an.TIE_SETS:
        assert list(copies) == sorted(set(copies)) and copies[-1] < M and d % 16 == 0
        inp = an.tie_inputs((M, d, copies))
        W, anchors = inp["W"], inp["anchors"]
        assert all(np.array_equal(W[j], W[copies[0]]) for j in copies)
        assert (np.unique(W, axis=0).shape[0]) == M - len(copies) + 1          # no other duplicates
        assert np.array_equal(anchors[an.TIE_ANCHOR], W[copies[0]]) and anchors.shape[0] == an.TIE_A == 17


# ---- the references alone stay inside the caps of the GPU file -------------------------------------------------------
@pytest.mark.parametrize("row", an.SEED_ROWS, ids=an.seed_row_id)
def test_reference_argmin_is_unambiguous_on_every_row_of_the_table(row):
    N, _, (A, M, d, kind, dtype, buckets) = row
    inp = an.seed_inputs(row)
    X, W, anchors = inp["X"], inp["W"], inp["anchors"]
    assert X.shape == (N, d) and X.dtype == (np.float32 if dtype == "f32" else np.float64)
    assert W.shape == (M, d) and anchors.shape == (A, d) and anchors.dtype == np.float64
    assert np.isfinite(W).all() and np.unique(W, axis=0).shape[0] == M
    assert {tuple(r) for r in anchors} <= {tuple(r) for r in X.astype(np.float64)}
    aof, order = inp["anchor_of"], inp["order"]
    assert aof.dtype == order.dtype == np.int32 and aof.min() >= 0 and aof.max() < A
    assert np.array_equal(np.sort(order), np.arange(N)) and (np.diff(aof[order]) >= 0).all()
    ref = an.argmin_reference(anchors, W)
    # the reference's own arg-min passes every check (0 ambiguous anchors is one of them) ...
    n_eq = an.check_argmin(ref[0].argmin(axis=1), anchors, W, ref)
    assert n_eq == A
    # ... and the checks are not vacuous: the runner-up fails them wherever there is one
    if M > 1:
        second = np.argsort(ref[0], axis=1, kind="stable")[:, 1]
        with pytest.raises(AssertionError):
            an.check_argmin(second, anchors, W, ref)
    # float64 is close to the bound's scale, not orders beyond it
    v64 = (W * W).sum(axis=1)[None, :] - 2.0 * (anchors @ W.T)
    assert (np.abs(v64.astype(an.L) - ref[0]) <= ref[1]).all()


@pytest.mark.parametrize("kind", an.SEED_KINDS)
@pytest.mark.parametrize("N,d,M", [(300, 16, 63), (1000, 48, 65), (1000, 80, 130), (2000, 320, 1985), (4096, 64, 4100)])
def test_reference_argmin_is_unambiguous_at_the_context_shapes(N, d, M, kind):
    """prototypes as sample rows plus 0.05 noise, anchors as the engine picks and chains them: 0 ambiguous anchors"""
    import bench

    X = bench.make_shard_numpy(N, d, 1000 + N + d + M, kind=kind).astype(np.float64)
    A = min(256, N)
    anchors = X[an.anchor_rows(N, A)]
    anchors = anchors[an.chain(anchors)]
    rng = np.random.default_rng(3)
    W = X[rng.choice(N, M, replace=M > N)] + 0.05 * rng.standard_normal((M, d))
    ref = an.argmin_reference(anchors, W)
    assert an.check_argmin(ref[0].argmin(axis=1), anchors, W, ref) == A


@pytest.mark.parametrize("M,d,every_row", [(130, 48, False), (1985, 16, False), (20, 48, True)])
def test_reference_with_non_finite_rows(M, d, every_row):
    inp = an.bad_inputs(M, d, every_row)
    W, anchors = inp["W"], inp["anchors"]
    fin = an.finite_rows(W)
    assert fin.sum() == (0 if every_row else M - 3)
    kinds = [np.isnan(W[j]).any() for j in range(M) if not fin[j]], [np.isinf(W[j]).any() for j in range(M) if not fin[j]]
    assert any(kinds[0]) and any(kinds[1]) and any(np.isfinite(W[j]).all() for j in range(M) if not fin[j])
    if every_row:
        an.check_argmin(np.zeros(anchors.shape[0], dtype=np.int32), anchors, W)
        with pytest.raises(AssertionError):
            an.check_argmin(np.ones(anchors.shape[0], dtype=np.int32), anchors, W)
        return
    ref = an.argmin_reference(anchors, W)
    assert an.check_argmin(ref[0].argmin(axis=1), anchors, W, ref) == anchors.shape[0]
    bad = ref[0].argmin(axis=1).copy()
    bad[5] = 0                                            # the NaN row
    with pytest.raises(AssertionError):
        an.check_argmin(bad, anchors, W, ref)


@pytest.mark.parametrize("storage", an.CTX_STORAGE)
@pytest.mark.parametrize("N", [n for n in an.CTX_N if n > 256])
def test_emulated_buckets_pass_their_own_checks(N, storage):
    import bench

    X = bench.make_shard_numpy(N, an.CTX_D, 2000 + N)
    Xs = np.asarray(da.widen(da.stored(X, {"float32": "f32", "float64": "f64", "bf16": "bf16"}[storage])), dtype=np.float64)
    Xp = np.zeros((N, 80))
    Xp[:, :an.CTX_D] = Xs
    anchors = Xp[an.anchor_rows(N, 256)]
    anchors = anchors[an.chain(anchors)]
    aof, r, eps = an.emulated_buckets(Xp, anchors)
    an.check_buckets(aof, np.argsort(aof, kind="stable"), r, eps, 256)
    excess, share = an.bucket_quality(r, aof)
    print(f"N={N} {storage}: emulated buckets excess {excess:.4f}, {100 * share:.1f} % at the exact nearest anchor")
    assert excess >= 0.0
    # an anchor is a sample: it sits in its own bucket or in that of an anchor within 2 eps
    exact = r.argmin(axis=1)
    assert an.bucket_quality(r, exact) == (0.0, 1.0)
    with pytest.raises(AssertionError):
        an.check_buckets((exact + 1) % 256, np.argsort((exact + 1) % 256, kind="stable"), r, eps * 0, 256)


# ---- argument errors that return before any HIP call ------------------------------------------------------------------
P = 0x10000          # a fake, 256-byte aligned device address: never dereferenced on these paths


def _anchored(lib, *, A=16, M=130, stride=an.PRUNE, anchors=P, anchor_of=P, order=P, N=300, d=16):
    need = lib.dbgsom_bmu_filtered_workspace_bytes(N, d, M)
    return lib.dbgsom_bmu_filtered_anchored(P, da.F32, N, d, d, P, P, P, M, P, anchors, A, anchor_of, order, stride, 0, 0, P, P,
                                            P, need, None)


def test_argument_errors_of_the_anchor_entry_points(lib):
    def failed(rc, code, what=b""):
        msg = lib.dbgsom_last_error()
        assert rc == code and what in msg, (rc, msg)

    EINVAL = -1
    failed(_anchored(lib, A=0), EINVAL, b"anchor seeds")
    failed(_anchored(lib, A=257), EINVAL, b"anchor seeds")
    failed(_anchored(lib, stride=0), EINVAL, b"anchor seeds")                       # no DBGSOM_PRUNE
    failed(_anchored(lib, stride=an.PRUNE | an.SEED_FULL), EINVAL, b"anchor seeds")
    failed(_anchored(lib, M=8193), EINVAL, b"anchor seeds")                         # (DBGSOM_PRUNE is ignored there)
    failed(_anchored(lib, anchor_of=None), EINVAL, b"null anchor_of")
    failed(_anchored(lib, anchors=None), EINVAL, b"anchor seeds")
    failed(_anchored(lib, order=None), EINVAL, b"anchor seeds")
    failed(_anchored(lib, anchors=P + 8), EINVAL, b"alignment")
    failed(_anchored(lib, d=24), EINVAL, b"multiple of 16")
    aseed = np.zeros(256, dtype=np.int32)
    failed(lib.dbgsom_bmu_filtered_anchor_seeds(P, 300, 16, 8193, 16, aseed.ctypes.data, None, None), EINVAL, b"8192")
    failed(lib.dbgsom_bmu_filtered_anchor_seeds(P, 300, 16, 130, 0, aseed.ctypes.data, None, None), EINVAL, b"n_anchors")
    failed(lib.dbgsom_bmu_filtered_anchor_seeds(P, 300, 16, 130, 257, aseed.ctypes.data, None, None), EINVAL, b"n_anchors")
    failed(lib.dbgsom_bmu_filtered_anchor_seeds(None, 300, 16, 130, 16, aseed.ctypes.data, None, None), EINVAL, b"null pointer")
    failed(lib.dbgsom_bmu_filtered_anchor_seeds(P, 300, 16, 130, 16, None, None, None), EINVAL, b"null pointer")
    failed(lib.dbgsom_ctx_read_anchors(None, None, None, None, None, None), EINVAL, b"null context")
