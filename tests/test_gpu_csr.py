"""MI355X: CSR samples through the CSR kernels (csrc/csr.hip) against the oracle's chain on the densified matrix
and against the dense kernels on ``X.toarray()`` -- bit for bit -- and whole fits on sparse input against the
CPU stand-in's fit of the same input.  Option "csr_densify_below" is 0 wherever the CSR kernels are the subject."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import golden_inputs as gi
from tests.test_csr_cpu import CsrOracleBackend, digits_csr, topics, uncanonical

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _csr_backend(X=None, **kw):
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0, **kw)
    be.csr_densify_below = 0
    if X is not None:
        be.load(X)
        assert be.resident_csr
    return be


def _variants():
    """(name, CSR matrix): (ii) topics at d = 2048, (iii) d = 4096 and d = 1000 with N not a multiple of 128, empty
    rows, explicitly stored zeros and a block of columns nobody uses; float64 and float32."""
    out = []
    for dt in (np.float64, np.float32):
        n = np.dtype(dt).name
        out.append((f"topics2048-{n}", topics(dtype=dt)[0]))
        out.append((f"topics4096-{n}", topics(N=1101, d=4096, dtype=dt, seed=4, empty_rows=23, stored_zeros=90,
                                              unused_tail=300)[0]))
        out.append((f"topics1000-{n}", topics(N=1303, d=1000, dtype=dt, seed=5, empty_rows=17, stored_zeros=70,
                                              unused_tail=64)[0]))
    return out


def _prototypes(X, M, seed=11):
    """M prototypes near rows of X (dense float64), with a NaN row and duplicate rows when the map is large enough."""
    rng = np.random.default_rng(seed)
    D = X[np.sort(rng.choice(X.shape[0], min(M, X.shape[0]), replace=False))].toarray().astype(np.float64)
    W = D[rng.integers(0, D.shape[0], M)] + rng.normal(0, 0.05, (M, X.shape[1]))
    if M >= 33:
        W[7] = np.nan          # never wins
        W[20] = W[3]           # ties go to the lowest index
        W[M - 1] = W[5]
    return W


@pytest.mark.parametrize("name,X", _variants(), ids=[n for n, _ in _variants()])
def test_csr_search_equals_the_chain_on_the_densified_matrix(name, X):
    from oracle import som_oracle as o

    D = X.toarray()
    be = _csr_backend(X)
    other = _csr_backend()
    messy = uncanonical(X)
    for M in (1, 2, 33, 256, 1024, 4000):
        for wdt in ((np.float64, np.float32) if X.dtype == np.float32 else (np.float64,)):
            W = _prototypes(X, M).astype(wdt)
            ks = (1,) if M == 1 else (1, 2)
            want_d2, want_i2 = o.bmu_chain(D, W, max(ks))
            if max(ks) == 1:
                want_d2, want_i2 = want_d2.reshape(-1, 1), want_i2.reshape(-1, 1)
            for k in ks:
                wd, wi = (want_d2[:, 0], want_i2[:, 0]) if k == 1 else (want_d2, want_i2)
                for what, (dist, idx) in (("resident", be.bmu(W, k)), ("query", other.bmu(W, k, X=X))):
                    assert np.array_equal(idx, wi), (name, M, wdt, k, what)
                    assert np.array_equal(dist, wd, equal_nan=True), (name, M, wdt, k, what)
        if M == 256:    # an unsorted matrix with duplicated entries is made canonical by the loader
            dist, idx = other.bmu(W, 2, X=messy)
            assert np.array_equal(idx, want_i2) and np.array_equal(dist, want_d2, equal_nan=True)
    be.release()
    other.release()


def _pair(X, **kw):
    """(CSR resident, dense resident of X.toarray() with the all-pairs search)"""
    from dbgsom_amd.backend import HipBackend

    return _csr_backend(X, **kw), HipBackend(0, algorithm="exact").load(X.toarray())


def _same_epoch(a, b):
    if a.new_weights is not None:      # (None with keep_on_device: compared through get_weights)
        assert np.array_equal(a.new_weights, b.new_weights, equal_nan=True)
    assert np.array_equal(a.errors, b.errors) and np.array_equal(a.activations, b.activations)
    assert a.change_total == b.change_total or (np.isnan(a.change_total) and np.isnan(b.change_total))
    if a.winners is not None:
        assert np.array_equal(a.winners, b.winners) and np.array_equal(a.distances, b.distances)
    if a.class_hist is not None:
        assert np.array_equal(a.class_hist, b.class_hist)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [2048, 4096])
def test_csr_sums_and_epoch_equal_the_dense_kernels(d, dtype):
    from dbgsom_amd.backend import RESIDENT

    X, y = topics(dtype=dtype) if d == 2048 else topics(N=1101, d=4096, dtype=dtype, seed=4, empty_rows=23,
                                                        stored_zeros=90, unused_tail=300)
    rows, cols = 9, 11
    M = rows * cols
    W = _prototypes(X, M)
    W[7] = W[8] + 1e3                      # (no NaN row here: a dead neuron instead)
    hop = gi.lattice_hops(rows, cols)
    gamma = 1.0 / float(np.var(X.toarray().astype(np.float64), axis=0).sum())
    cs, dn = _pair(X)
    ra, rb = cs.epoch(W, hop, 1.4, gamma, "compact", True), dn.epoch(W, hop, 1.4, gamma, "compact", True)
    _same_epoch(ra, rb)
    assert np.array_equal(cs.read_sums(M), dn.read_sums(M))
    assert (ra.activations == 0).any()
    # update with the caller's winners / sample weights
    kw = np.random.default_rng(2).random(X.shape[0])
    ua = cs.update(W, hop, 1.4, kw, ra.winners, ra.distances, "aligned")
    ub = dn.update(W, hop, 1.4, kw, rb.winners, rb.distances, "aligned")
    for p, q in zip(ua, ub):
        assert np.array_equal(p, q)
    # class histograms of the entropy criterion
    for be in (cs, dn):
        be.set_labels(y.astype(np.int32))
    _same_epoch(cs.epoch(W, hop, 1.4, gamma, "compact", True, n_classes=10),
                dn.epoch(W, hop, 1.4, gamma, "compact", True, n_classes=10))
    # three epochs in a row on the resident prototypes
    for be in (cs, dn):
        be.set_weights(W)
    for _ in range(3):
        _same_epoch(cs.epoch(RESIDENT, hop, 1.2, gamma, "compact", True, keep_on_device=True),
                    dn.epoch(RESIDENT, hop, 1.2, gamma, "compact", True, keep_on_device=True))
    assert np.array_equal(cs.get_weights(0), dn.get_weights(0))
    # sample weights, zeros among them
    w = np.random.default_rng(7).integers(0, 4, X.shape[0]).astype(np.float64)
    for be in (cs, dn):
        be.set_sample_weight(w)
    _same_epoch(cs.epoch(W, hop, 1.4, gamma, "compact", True, n_classes=10),
                dn.epoch(W, hop, 1.4, gamma, "compact", True, n_classes=10))
    assert np.array_equal(cs.read_sums(M), dn.read_sums(M))
    ua = cs.update(W, hop, 1.4, kw, ra.winners, ra.distances)
    ub = dn.update(W, hop, 1.4, kw, rb.winners, rb.distances)
    for p, q in zip(ua, ub):
        assert np.array_equal(p, q)
    assert cs.quantization_error(W) == dn.quantization_error(W)
    assert np.array_equal(cs.node_statistics(W, 1.3)[1], dn.node_statistics(W, 1.3)[1])
    cs.release()
    dn.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reductions_on_a_csr_resident_equal_the_dense_backend(dtype):
    from dbgsom_amd import _native

    X, _ = topics(N=1303, d=2048, dtype=dtype, seed=6, empty_rows=9, stored_zeros=40)
    rows, cols = 12, 13
    M = rows * cols
    W = _prototypes(X, M)
    coords = [(i, j) for i in range(rows) for j in range(cols)]
    cs, dn = _pair(X)
    assert cs.quantization_error(W) == dn.quantization_error(W)
    assert cs.topographic_error_count(W, coords) == dn.topographic_error_count(W, coords)
    for p, q in zip(cs.node_statistics(W, 1.3), dn.node_statistics(W, 1.3)):
        assert np.array_equal(p, q)
    (ca, wa), (cb, wb) = cs.partition(W, want_winners=True), dn.partition(W, want_winners=True)
    assert np.array_equal(ca, cb) and np.array_equal(wa, wb)
    pick = np.array([0, 5, 1302, 77, 5])
    assert np.array_equal(cs.read_samples(pick), X[pick].toarray().astype(np.float64))
    assert np.array_equal(cs.read_samples(pick), dn.read_samples(pick))
    # what a CSR resident does not offer is refused with a message, not computed some other way
    with pytest.raises(_native.DbgsomNativeError, match="CSR"):
        cs.subset(3)
    assert cs.column_moments() is None
    with pytest.raises(ValueError):
        cs.load(X, storage="bf16")
    cs.release()
    dn.release()


def test_narrow_csr_input_is_densified_on_the_device():
    from dbgsom_amd import SomVQ
    from dbgsom_amd.backend import HipBackend

    Xs, _ = digits_csr()
    be = HipBackend(0)
    assert be.csr_densify_below == 1024
    be.load(Xs)
    assert not be.resident_csr and be.padded_features == 64
    assert np.array_equal(be.read_samples(np.arange(50)), Xs[:50].toarray())
    W = _prototypes(Xs, 40)
    dn = HipBackend(0).load(Xs.toarray())
    for p, q in zip(be.bmu(W, 2), dn.bmu(W, 2)):
        assert np.array_equal(p, q, equal_nan=True)
    for p, q in zip(be.bmu(W, 2, X=Xs[:333]), dn.bmu(W, 2, X=Xs[:333].toarray())):
        assert np.array_equal(p, q, equal_nan=True)
    dn.release()
    be.load(topics()[0])
    assert be.resident_csr                               # d = 2048: stays CSR
    be.release()
    a = SomVQ(random_state=0).fit(Xs)
    b = SomVQ(random_state=0).fit(Xs.toarray())
    assert a.n_iter_ == b.n_iter_ and a.neurons_ == b.neurons_ and np.array_equal(a.labels_, b.labels_)
    diff = float(np.abs(a.weights_ - b.weights_).max() / np.abs(b.weights_).max())
    print(f"digits CSR (densified on the device) against dense: max |dW| / max |W| = {diff:.2e}")
    assert diff <= 1e-12                                 # (the float64 gate of tests/test_csr_cpu.py: the moments)


@pytest.mark.parametrize("case", ["topics2048-vq", "topics4096-entropy", "topics2048-vertical"])
def test_whole_fits_on_the_csr_kernels_match_the_cpu_stand_in(case):
    from dbgsom_amd import SomClassifier, SomVQ

    kw = dict(n_iter=40, max_neurons=40, random_state=0)
    if case.startswith("topics4096"):
        X, y = topics(N=1101, d=4096, seed=4, empty_rows=23, stored_zeros=90, unused_tail=300)
    else:
        X, y = topics()
    if case.endswith("vq"):
        mk = lambda **b: SomVQ(**kw, **b)                                              # noqa: E731
        y = None
    elif case.endswith("entropy"):
        mk = lambda **b: SomClassifier(growth_criterion="entropy", spreading_factor=0.4, **kw, **b)   # noqa: E731
    else:
        mk = lambda **b: SomClassifier(vertical_growth=True, min_samples_vertical_growth=200,          # noqa: E731
                                       **dict(kw, max_neurons=12), **b)
    gpu = mk(backend=_csr_backend()).fit(X, y)
    cpu = mk(backend=CsrOracleBackend()).fit(X, y)
    assert gpu.neurons_ == cpu.neurons_ and gpu.n_iter_ == cpu.n_iter_
    np.testing.assert_allclose(gpu.weights_, cpu.weights_, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(gpu.quantization_error_, cpu.quantization_error_, rtol=1e-8, atol=1e-10)
    assert gpu.topographic_error_ == cpu.topographic_error_
    if y is None:
        assert np.array_equal(gpu.labels_, cpu.labels_)
        assert np.array_equal(gpu.predict(X[:500]), cpu.predict(X[:500]))
    else:
        assert np.array_equal(gpu._extract_values_from_graph("label"), cpu._extract_values_from_graph("label"))
        dense = gpu.predict_proba(X[:700].toarray())
        # (an empty row has no direction: its probabilities are NaN, as for a dense row of zeros)
        assert np.array_equal(gpu.predict_proba(X[:700]), dense, equal_nan=True)
        gpu._SPARSE_CODE_ROWS = 300      # several chunks: rows are coded independently, bit for bit on the device
        assert np.array_equal(gpu.predict_proba(X[:700]), dense, equal_nan=True)
    if case.endswith("vertical"):
        kids = [n for n, at in gpu.som_.nodes.items() if "som" in at]
        assert kids == [n for n, at in cpu.som_.nodes.items() if "som" in at] and kids
        for n in kids:
            assert gpu.som_.nodes[n]["som"].neurons_ == cpu.som_.nodes[n]["som"].neurons_


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[5])
rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
import torch.distributed as td
td.init_process_group("gloo", rank=rank, world_size=world)
from dbgsom_amd import SomVQ
from dbgsom_amd.backend import HipBackend
from tests.test_csr_cpu import topics
X, _ = topics()
be = HipBackend(0)
be.csr_densify_below = 0
est = SomVQ(n_iter=40, max_neurons=40, random_state=0, backend=be).fit(X)   # every rank loads its CSR row slice
np.savez(out, weights=est.weights_, labels=est.labels_, n_iter=est.n_iter_, neurons=np.array(est.neurons_),
         qe=est.quantization_error_, te=est.topographic_error_)
td.barrier()
td.destroy_process_group()
'''


def test_two_ranks_each_with_its_csr_row_slice(tmp_path):
    from dbgsom_amd import SomVQ

    world, port = 2, _free_port()
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), port, outs[r], os.path.dirname(HERE)],
                              env=env) for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=600) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    res = [np.load(o) for o in outs]
    X, _ = topics()
    one = SomVQ(n_iter=40, max_neurons=40, random_state=0, backend=_csr_backend()).fit(X)
    assert np.array_equal(res[0]["weights"], res[1]["weights"])           # ranks agree bit for bit
    for r in res:
        assert [tuple(n) for n in r["neurons"]] == one.neurons_ and int(r["n_iter"]) == one.n_iter_
        assert np.array_equal(r["labels"], one.labels_)
        np.testing.assert_allclose(r["weights"], one.weights_, rtol=1e-9, atol=1e-11)   # (tests/test_gpu_distributed.py)
        np.testing.assert_allclose(float(r["qe"]), one.quantization_error_, rtol=1e-12)
        assert float(r["te"]) == one.topographic_error_


def zipf_csr(N, d, per_row, seed=0, dtype=np.float32):
    """N rows of about `per_row` stored entries, columns drawn with a Zipf-like popularity (tools/bench_csr.py)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, d + 1) ** 0.9
    cdf = np.cumsum(p / p.sum())
    cols = np.minimum(np.searchsorted(cdf, rng.random(N * per_row)), d - 1).astype(np.int64)
    key = np.unique(np.repeat(np.arange(N, dtype=np.int64), per_row) * d + rng.permutation(d)[cols])
    rows, cols = key // d, (key % d).astype(np.int32)
    indptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=N))].astype(np.int64)
    return sp.csr_matrix((rng.gamma(2.0, 1.0, key.size).astype(dtype), cols, indptr), shape=(N, d))


def _big_epoch():
    from dbgsom_amd import _native

    N, d, M = 200000, 50000, 256
    X = zipf_csr(N, d, 100)
    be = _csr_backend(X)
    W = X[np.random.default_rng(1).choice(N, M, replace=False)].toarray().astype(np.float64)
    res = be.epoch(W, gi.lattice_hops(16, 16), 2.0, 1e-3, "compact", False, keep_on_device=True)
    assert res.activations.sum() == N
    used = be._get("device_bytes")
    lib = _native.load()
    dp = be.padded_features
    terms = {"csr": X.data.nbytes + X.indices.size * 4 + (N + 1) * 8, "Wt": dp * lib.dbgsom_csr_wt_ld(M) * 8,
             "W": 2 * M * dp * 8, "accumulate": lib.dbgsom_accumulate_csr_workspace_bytes(N, dp, M),
             "smooth": lib.dbgsom_smooth_workspace_bytes(M, dp), "rows": 64 * N}
    be.release()
    return used, terms, N * d * 4, M * (dp + 3) * 8


def test_nothing_of_size_n_times_d_is_allocated_for_a_csr_resident():
    """"device_bytes" after loading 2e5 x 50 000 (100 per row) and one epoch at M = 256 stays below the CSR arrays
    + Wt + the two W buffers + the accumulate and smoothing workspaces as the library's *_workspace_bytes functions
    report them + 64 bytes per row -- from the shapes alone -- and far below the 40 GB of the dense float32 form.
    (The buffer of the reduced sums, M x (d + 3) float64, is not in that list: a context with a CSR resident
    allocates without head room and runs the smoothing inside the accumulate workspace, whose slab is dead by
    then, to stay below it.)"""
    used, terms, dense, _ = _big_epoch()
    bound = sum(terms.values())
    print(f"device_bytes {used / 1e6:.1f} MB, bound {bound / 1e6:.1f} MB ({terms}), dense float32 {dense / 1e9:.1f} GB")
    assert used < dense / 20
    assert used < bound
