"""GPU: ``fit(X, y, sample_weight=w)`` from the weighted epoch kernels (accumulate.hip, stats.hip) up to the
estimators.  A row of weight w counts as w copies of that row, so for integer weights everything is checked
against the unweighted oracle / the reference's recorded fits on ``np.repeat(X, w, axis=0)``.  Tolerances are
the ones tests/test_gpu_parity.py and tests/test_gpu_estimator.py apply to the same quantities."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_inputs as gi
from tests import golden_inputs_weighted as giw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
TV = np.float64(1000.0)   # total variance of the epoch tests: gamma = 1 / TV = 1e-3 exactly as the literal


@pytest.fixture(scope="module")
def o():
    from oracle import som_oracle

    return som_oracle


def _data(N, d, M, dt, seed):
    """-> (X as stored, X as the device sees it, storage, W, hop, w): blobs, a map of M of their rows, integer
    weights 0 .. 3 with a fifth of the rows at 0"""
    rng = np.random.default_rng(seed)
    X, _ = gi.blobs_f32(N, d, seed, n_centers=12)
    storage = None
    Xr = X
    if dt == "f64":
        X = Xr = X.astype(np.float64) * 1.0000001
    elif dt == "bf16":
        import torch

        storage = "bf16"
        Xr = torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    W = X[rng.choice(N, M, replace=False)].astype(np.float64)
    hop = np.abs(np.subtract.outer(np.arange(M), np.arange(M))).astype(np.float64)
    w = rng.integers(0, 4, N).astype(np.float64)
    w[rng.random(N) < 0.2] = 0.0
    return X, Xr, storage, W, hop, w


def _split(sums, M, d):
    return sums[:M * d].reshape(M, d), sums[M * d:M * d + M], sums[M * d + M:M * d + 2 * M], sums[M * d + 2 * M:]


def _check_against_repeated_rows(o, be, Xr, W, hop, w, sigma, tv, ref_win, ref_dist):
    """one frozen weighted epoch of `be` against the oracle's unweighted epoch on np.repeat(X, w, 0)"""
    M, d = W.shape
    gamma = float(tv ** -1)
    res = be.epoch(W, hop, sigma, gamma, "compact", True, frozen=True)
    assert np.array_equal(res.winners, ref_win)       # the search does not depend on weights
    assert np.array_equal(res.distances, ref_dist)
    S, K, a, E = _split(be.read_sums(M), M, d)
    wi = w.astype(np.int64)
    Xrep = np.repeat(Xr, wi, axis=0)
    oo = o.epoch(Xrep, W, hop, sigma, tv, "compact", "chain")
    assert np.array_equal(oo.winners, np.repeat(ref_win, wi)) and np.array_equal(oo.distances, np.repeat(ref_dist, wi))
    So, Ko, ao, Eo = o.accumulate(Xrep, oo.winners, oo.sample_weights, oo.distances, M)
    assert np.array_equal(a, np.bincount(ref_win, weights=w, minlength=M))   # sums of small integers: exact
    assert np.array_equal(a, ao) and np.array_equal(res.activations, ao)
    np.testing.assert_allclose(E, Eo, rtol=1e-12)
    np.testing.assert_allclose(res.errors, oo.errors, rtol=1e-12)
    np.testing.assert_allclose(K, Ko, rtol=1e-12)
    # S: two orders of additions of the same terms w h x -- the oracle adds a_j of them, the kernel at most as many
    # rows, each with one more rounding (w h); a sum of n terms is within n u sum |terms| of the exact one.  The
    # factor h itself is the device's exp / sqrt against NumPy's: rtol 1e-13 (test_gpu_parity.py, exp_similarity)
    Sabs = o.accumulate(np.abs(Xrep), oo.winners, oo.sample_weights, oo.distances, M)[0]
    assert np.all(np.abs(S - So) <= ((2 * ao[:, None] + 2) * U + 1e-13) * Sabs)
    np.testing.assert_allclose(res.new_weights, oo.new_weights, rtol=1e-11, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(res.change_total, oo.change_total, rtol=1e-9, atol=1e-12)
    assert np.all(S[a == 0] == 0) and np.all(K[a == 0] == 0) and np.all(E[a == 0] == 0)   # dead by weight: exact zeros
    return res


# shapes of segsum_kernel: narrow rows with row lanes (d = 37 too: the context pads it to 48, so it takes the vector
# loads and row lanes -- the scalar instantiations are run by tests/test_gpu_device_abi.py) / wide rows; M on both
# sides of the second-level sum of finalize_kernel (finalize_groups: M <= 256) and of 512
@pytest.mark.parametrize("dt,N,d,M", [("f32", 6000, 48, 30), ("f64", 5000, 37, 300), ("bf16", 7000, 64, 600),
                                      ("f32", 3000, 1040, 140)])
def test_weighted_epoch_matches_the_oracle_on_repeated_rows(o, dt, N, d, M):
    from dbgsom_amd.backend import HipBackend

    X, Xr, storage, W, hop, w = _data(N, d, M, dt, N + d + M)
    be = HipBackend(algorithm="exact").load(X, storage=storage)
    r0 = be.epoch(W, hop, 1.5, 1e-3, "compact", True, frozen=True)      # unweighted
    for j in np.flatnonzero(r0.activations > 0)[:3]:                    # neurons whose rows all have weight 0
        w[r0.winners == j] = 0.0
    assert (w == 0).sum() > N // 10
    be.set_sample_weight(w)
    r1 = _check_against_repeated_rows(o, be, Xr, W, hop, w, 1.5, TV, r0.winners, r0.distances)
    # determinism: the same bits twice
    r2 = be.epoch(W, hop, 1.5, 1e-3, "compact", True, frozen=True)
    assert np.array_equal(r1.new_weights, r2.new_weights, equal_nan=True) and np.array_equal(r1.errors, r2.errors)
    assert np.array_equal(r1.activations, r2.activations) and r1.change_total == r2.change_total
    # detached again: the unweighted epoch, bit for bit
    be.set_sample_weight(None)
    r3 = be.epoch(W, hop, 1.5, 1e-3, "compact", True, frozen=True)
    assert np.array_equal(r3.new_weights, r0.new_weights, equal_nan=True) and np.array_equal(r3.activations, r0.activations)
    be.release()


# the weighted epoch behind the refined search (refinement, pair kernel, then the weighted segsum_kernel): rows
# narrower and wider than a workgroup's column groups, three storage types, M on both sides of the second-level sum
@pytest.mark.parametrize("dt,d,M", [("f32", 256, 200), ("f64", 320, 300), ("bf16", 4096, 200), ("f32", 1280, 600)])
def test_weighted_epoch_behind_the_refined_search(o, dt, d, M):
    from dbgsom_amd.backend import HipBackend

    N = 9003
    X, Xr, storage, W, hop, w = _data(N, d, M, dt, d + M)
    W[7] = W[3]
    ex = HipBackend(algorithm="exact").load(X, storage=storage)
    r0 = ex.epoch(W, hop, 1.5, 1e-3, "compact", True, frozen=True)
    for j in np.flatnonzero(r0.activations > 0)[:3]:
        w[r0.winners == j] = 0.0
    ex.set_sample_weight(w)
    re_ = ex.epoch(W, hop, 1.5, 1e-3, "compact", True, frozen=True)      # weighted, segsum_kernel
    fi = HipBackend(algorithm="filtered").load(X, storage=storage)
    fi.refine, fi.sweep_planes = 1, 4
    fi.set_sample_weight(w)
    rf = _check_against_repeated_rows(o, fi, Xr, W, hop, w, 1.5, TV, r0.winners, r0.distances)
    assert fi.filter_log[-1][0] == "filtered" and fi.refined
    # the refined and the exact backend's weighted epochs leave the same bits
    assert np.array_equal(rf.new_weights, re_.new_weights, equal_nan=True)
    assert np.array_equal(rf.errors, re_.errors) and np.array_equal(rf.activations, re_.activations)
    rf2 = fi.epoch(W, hop, 1.5, 1e-3, "compact", True, frozen=True)
    assert np.array_equal(rf2.new_weights, rf.new_weights, equal_nan=True) and np.array_equal(rf2.errors, rf.errors)
    ex.release()
    fi.release()


@pytest.mark.parametrize("dt,N,d,M", [("f32", 6000, 48, 30), ("f64", 5000, 64, 300)])
def test_fractional_weights_and_scale_invariance(dt, N, d, M):
    """Fractional weights against a float64 NumPy restatement (rows sorted by winner, np.add.reduceat); w and
    2 w give bit-identical prototypes (a power of two scales every partial exactly) and errors scaled by 2."""
    from dbgsom_amd.backend import HipBackend
    from oracle import som_oracle as o

    X, Xr, storage, W, hop, w = _data(N, d, M, dt, 5 * N + M)
    rng = np.random.default_rng(1)
    w = w * rng.uniform(0.1, 2.5, N)
    gamma, sigma = 1e-3, 1.5
    be = HipBackend(algorithm="exact").load(X, storage=storage)
    r0 = be.epoch(W, hop, sigma, gamma, "compact", True, frozen=True)
    be.set_sample_weight(w)
    r1 = be.epoch(W, hop, sigma, gamma, "compact", True, frozen=True)
    S, K, a, E = _split(be.read_sums(M), M, d)
    assert np.array_equal(r1.winners, r0.winners) and np.array_equal(r1.distances, r0.distances)
    keep = w > 0
    win, dist, wk = r0.winners[keep], r0.distances[keep], w[keep]
    order = np.argsort(win, kind="stable")
    win, dist, wk, Xs = win[order], dist[order], wk[order], Xr[keep][order].astype(np.float64)
    h = o.exp_similarity_gamma(dist, gamma)
    ids, starts = np.unique(win, return_index=True)

    def seg(v):
        out = np.zeros((M,) + v.shape[1:])
        out[ids] = np.add.reduceat(v, starts, axis=0)
        return out

    f = wk * h
    So, Ko, ao, Eo = seg(f[:, None] * Xs), seg(f), seg(wk), seg(wk * dist)
    np.testing.assert_allclose(a, ao, rtol=1e-12)
    np.testing.assert_allclose(K, Ko, rtol=1e-12)
    np.testing.assert_allclose(E, Eo, rtol=1e-12)
    n = np.bincount(win, minlength=M)[:, None]
    assert np.all(np.abs(S - So) <= ((2 * n + 4) * U + 1e-13) * seg(f[:, None] * np.abs(Xs)))   # (as above, n rows on both sides)
    Wo = o.smooth_matmul(o.gaussian_neighborhood(hop, sigma), ao, o.voronoi_centers(So, Ko, ao, "compact"))
    np.testing.assert_allclose(r1.new_weights, Wo, rtol=1e-11, atol=1e-12, equal_nan=True)
    be.set_sample_weight(2.0 * w)
    r2 = be.epoch(W, hop, sigma, gamma, "compact", True, frozen=True)
    assert np.array_equal(r2.new_weights, r1.new_weights, equal_nan=True)
    assert np.array_equal(r2.errors, 2.0 * r1.errors) and np.array_equal(r2.activations, 2.0 * r1.activations)
    be.release()


def test_weighted_reductions_against_numpy():
    """QE, topographic weight, hit counts / density sums, class histogram and column moments with weights."""
    from dbgsom_amd.backend import HipBackend

    N, d, rows, cols = 7001, 40, 5, 6
    M = rows * cols
    X, Xr, _, W, _, w = _data(N, d, M, "f32", 77)
    y = (np.arange(N) % 5).astype(np.int32)
    be = HipBackend().load(X)
    dist2, idx2 = be.bmu(W, 2)
    dist, win = dist2[:, 0], idx2[:, 0]
    be.set_sample_weight(w)
    be.set_labels(y)
    wt = w.sum()
    assert be.weight_total() == wt
    np.testing.assert_allclose(be.quantization_error(W), (w @ dist) / wt, rtol=1e-12)
    coords = [(i, j) for i in range(rows) for j in range(cols)]
    pos = np.asarray(coords, dtype=np.float64)
    apart = np.linalg.norm(pos[idx2[:, 0]] - pos[idx2[:, 1]], axis=1) > 1.5
    assert be.topographic_error_count(W, coords) == w[apart].sum()          # integer weights: exact
    hits, dens = be.node_statistics(W, 1.3)
    assert np.array_equal(hits, np.bincount(win, weights=w, minlength=M))
    terms = np.exp(-(dist ** 2) / (2 * 1.3 ** 2)) / (1.3 * np.sqrt(2 * np.pi))
    np.testing.assert_allclose(dens, np.bincount(win, weights=w * terms, minlength=M), rtol=1e-12)
    hist = np.zeros((M, 5))
    np.add.at(hist, (win, y), w)
    h1 = be.class_histogram(win, 5, M)
    assert h1.dtype == np.float64 and np.array_equal(h1, hist)
    assert np.array_equal(be.class_histogram(win, 5, M), h1)
    s1, s2 = be.weighted_column_moments(wt)
    X64 = X.astype(np.float64)
    np.testing.assert_allclose(s1, w @ X64, rtol=1e-12)
    np.testing.assert_allclose(s2, w @ (X64 - s1 / wt) ** 2, rtol=1e-11)
    be.release()


def _compare_with_fixture(est, g, name, X, w):
    assert est.n_iter_ == int(g["final_n_iter"])
    assert [tuple(n) for n in g["final_neurons"]] == est.neurons_
    np.testing.assert_allclose(est.weights_, g["final_weights"], rtol=1e-5)
    np.testing.assert_allclose(est.weights_, g["final_weights"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(est.quantization_error_, float(g["final_qe"]), rtol=1e-10)
    assert est.topographic_error_ == float(g["final_te"])   # (integer weights: an exact count over an exact sum)
    np.testing.assert_allclose(est.growing_threshold_, float(g["final_growing_threshold"]), rtol=1e-12)
    assert np.array_equal(est._extract_values_from_graph("hit_count"), g["final_hit_count"])
    np.testing.assert_allclose(est._extract_values_from_graph("density"), g["final_density"], rtol=1e-8)   # (a function of weights_)
    if name in giw.CLF_CASES:
        assert np.array_equal(est._extract_values_from_graph("label"), g["final_node_label"])
        np.testing.assert_allclose(est._extract_values_from_graph("probabilities"), g["final_node_probabilities"],
                                   rtol=1e-12, atol=1e-15)
        assert np.array_equal(est._get_winning_neurons(X, n_bmu=1)[1], g["distinct_bmu"])
    else:
        assert np.array_equal(est.labels_, g["distinct_bmu"])               # BMUs of the distinct rows, weight 0 included
        assert np.array_equal(np.repeat(est.labels_, w), g["final_labels"])


@pytest.mark.parametrize("name", giw.FIT_CASES)
def test_weighted_fit_matches_the_reference_on_repeated_rows(name):
    from dbgsom_amd import SomClassifier, SomVQ
    from dbgsom_amd.backend import HipBackend

    g = giw.load(name)
    X, y, w = giw.case(name)
    cls = SomClassifier if name in giw.CLF_CASES else SomVQ
    est = cls(**giw.EST_KWARGS[name]).fit(X, y, sample_weight=w)
    assert isinstance(est._engine(), HipBackend)
    _compare_with_fixture(est, g, name, X, w)
    # the same fit on the repeated rows, unweighted, on the GPU as well
    Xr, yr = giw.repeated(name)
    rep = cls(**giw.EST_KWARGS[name]).fit(Xr, yr)
    assert rep.n_iter_ == est.n_iter_ and rep.neurons_ == est.neurons_
    np.testing.assert_allclose(est.weights_, rep.weights_, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(est.quantization_error_, rep.quantization_error_, rtol=1e-10)
    assert est.topographic_error_ == rep.topographic_error_
    assert np.array_equal(est._extract_values_from_graph("hit_count"), rep._extract_values_from_graph("hit_count"))
    if name not in giw.CLF_CASES:
        assert np.array_equal(cls(**giw.EST_KWARGS[name]).fit_predict(X, sample_weight=w), est.labels_)


def test_all_ones_weights_give_the_unweighted_fit():
    from dbgsom_amd import SomVQ

    name = "lowd_linear"
    g = gi.load(name)
    X, _ = gi.case_X(name)
    a = SomVQ(**gi.EST_KWARGS[name]).fit(X)
    b = SomVQ(**gi.EST_KWARGS[name]).fit(X, sample_weight=np.ones(len(X)))
    assert a.n_iter_ == b.n_iter_ == int(g["final_n_iter"]) and a.neurons_ == b.neurons_
    assert np.array_equal(a.labels_, b.labels_) and np.array_equal(b.labels_, g["final_labels"])
    np.testing.assert_allclose(b.weights_, a.weights_, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(b.weights_, g["final_weights"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(b.quantization_error_, float(g["final_qe"]), rtol=1e-10)
    assert b.topographic_error_ == float(g["final_te"])
    np.testing.assert_allclose(b.growing_threshold_, a.growing_threshold_, rtol=1e-12)


def test_vertical_growth_hands_the_weights_to_the_children():
    from dbgsom_amd import SomVQ

    name = giw.VERTICAL_CASE
    g = giw.load(name)
    X, _, w = giw.case(name)
    est = SomVQ(**giw.EST_KWARGS[name]).fit(X, sample_weight=w)
    paths = [list(g["paths_flat"][g["paths_off"][k]:g["paths_off"][k + 1]]) for k in range(int(g["n_maps"]))]
    seen = []

    def walk(e, path, wts):
        k = len(seen)
        seen.append(path)
        assert path == [int(v) for v in paths[k]], (path, paths[k])
        assert [tuple(n) for n in g[f"map{k}_neurons"]] == e.neurons_, path
        assert e.n_iter_ == int(g[f"map{k}_n_iter"]), path
        np.testing.assert_allclose(e.weights_, g[f"map{k}_weights"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(e.quantization_error_, float(g[f"map{k}_qe"]), rtol=1e-9)
        assert e.topographic_error_ == float(g[f"map{k}_te"]), path
        np.testing.assert_allclose(e.growing_threshold_, float(g[f"map{k}_threshold"]), rtol=1e-12)
        assert wts.sum() == int(g[f"map{k}_n_samples"])              # the map's rows, counted by weight
        for i, node in enumerate(e.neurons_):
            child = e.som_.nodes[node].get("som")
            if child is not None:
                walk(child, path + [i], wts[e.labels_ == i])

    walk(est, [], w)
    assert len(seen) == len(paths) > 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_two_ranks_with_their_rows_weights(tmp_path):
    from dbgsom_amd import SomClassifier, SomVQ

    world = 2
    port = _free_port()
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_dist_worker_weighted.py"), str(r), str(world), port,
                               outs[r]], env=env) for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    res = [np.load(f) for f in outs]
    for k in res[0].files:                                # the ranks agree bit for bit
        if not k.startswith("loc_labels"):
            assert np.array_equal(res[0][k], res[1][k], equal_nan=True), k
    name = "weighted_digits_vq"
    X, _, w = giw.case(name)
    one = SomVQ(**giw.EST_KWARGS[name]).fit(X, sample_weight=w)
    g = giw.load(name)
    for tag in ("fit", "loc"):
        r = res[0]
        assert int(r[f"{tag}_n_iter"]) == one.n_iter_ and [tuple(n) for n in r[f"{tag}_neurons"]] == one.neurons_
        np.testing.assert_allclose(r[f"{tag}_weights"], one.weights_, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(r[f"{tag}_weights"], g["final_weights"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(float(r[f"{tag}_qe"]), one.quantization_error_, rtol=1e-10)
        assert float(r[f"{tag}_te"]) == one.topographic_error_
    assert np.array_equal(res[0]["fit_labels"], one.labels_)
    assert np.array_equal(np.concatenate([r["loc_labels"] for r in res]), one.labels_)
    assert np.array_equal(res[0]["fit_hits"], one._extract_values_from_graph("hit_count"))
    name = "weighted_digits_entropy"
    X, y, w = giw.case(name)
    clf = SomClassifier(**giw.EST_KWARGS[name]).fit(X, y, sample_weight=w)
    assert int(res[0]["clf_n_iter"]) == clf.n_iter_ and [tuple(n) for n in res[0]["clf_neurons"]] == clf.neurons_
    np.testing.assert_allclose(res[0]["clf_weights"], clf.weights_, rtol=1e-8, atol=1e-10)
    assert np.array_equal(res[0]["clf_label"], clf._extract_values_from_graph("label"))


def test_bad_weights_are_status_codes():
    from dbgsom_amd import _native
    from dbgsom_amd.backend import HipBackend

    X, _ = gi.blobs_f32(500, 16, 3)
    be = HipBackend().load(X)
    lib = _native.load()
    for bad, what in ((np.ones(499), b"one weight per resident sample"),
                      (np.r_[np.ones(499), -1.0], b"negative or not finite"),
                      (np.r_[np.nan, np.ones(499)], b"negative or not finite"),
                      (np.r_[np.ones(499), np.inf], b"negative or not finite")):
        rc = lib.dbgsom_ctx_set_sample_weight(be._ctx, bad.ctypes.data_as(ctypes.c_void_p), bad.size)
        assert rc == -1 and what in lib.dbgsom_last_error(), (rc, lib.dbgsom_last_error())
    with pytest.raises(ValueError):
        be.set_sample_weight(-np.ones(500))
    be.set_sample_weight(np.ones(500))
    be.set_sample_weight(None)
    be.release()
