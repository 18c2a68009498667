"""MI355X: the stateless pruning search seeded from per-load anchor buckets (csrc/filter.hip 2e, option
"anchor_seeds").  The seeds only choose which candidate lists the exact stage walks: winners, distances and new
prototypes must be the all-pairs search's bit for bit, with the anchors and without them, at the shapes where the
anchor machinery takes another path (N below the 256 anchors, N no multiple of the 128-sample workgroup, maps that
are no multiple of the 64-prototype tile of the anchor-seed kernel), on degenerate anchors and on maps with
non-finite rows; the per-load state must be a function of the samples alone; and the seeds must be worth something
(lists of one cluster on well separated clusters).  `sweep_planes = 4` forces the pruning form and `seed_stride = 4`
(the library's own stride at these map sizes) keeps the policy on the cheap seeds the anchors replace -- left to
itself it may settle on the full pre-pass on a few thousand rows.  The anchors take over once the pre-pass has seeded
a settled pruning epoch of the sample set (the reference of their valve): the third epoch at the latest, so every
case runs four or more and asserts that the buckets were built and searches seeded from them."""
import numpy as np
import pytest

import bench
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu

MAPS = {130: (10, 13), 256: (16, 16)}
SIGMA = 1.1


def _backend(X, algorithm, anchors, storage=None, weights=None):
    from dbgsom_amd.backend import HipBackend

    be = HipBackend(0, algorithm=algorithm)
    be.anchor_seeds = anchors
    be.sweep_planes = 4
    be.seed_stride = 4
    be.load(X, storage=storage)
    if weights is not None:
        be.set_sample_weight(weights)
    return be


def _gamma(X):
    tv = float(np.asarray(X, dtype=np.float64).var(axis=0).sum())
    return 1.0 / tv if tv > 0 else 1.0


def _epochs(be, W0, M, gamma, frozen=3, evolving=3):
    """Three epochs from the same resident map (DBGSOM_EPOCH_FROZEN, the bench's path), then three in which the map
    evolves: every output of every epoch."""
    from dbgsom_amd.backend import RESIDENT

    hop = gi.lattice_hops(*MAPS[M])
    out, W = [], W0
    be.set_weights(W0)
    for e in range(frozen + evolving):
        if e < frozen:
            r = be.epoch(RESIDENT, hop, SIGMA, gamma, "compact", True, keep_on_device=True, frozen=True)
            Wn = be.get_weights(1)
        else:
            r = be.epoch(W, hop, SIGMA, gamma, "compact", True)
            Wn = W = r.new_weights
        out.append((r.winners, r.distances, Wn, r.errors, r.activations, np.array([r.change_total])))
    return out


def _same(a, b):
    for ea, eb in zip(a, b):
        for x, y in zip(ea, eb):
            if not np.array_equal(x, y, equal_nan=True):
                return False
    return len(a) == len(b)


def _three_ways(X, W0, M, storage=None, weights=None, **kw):
    """exact / anchors on / anchors off: bit-equal; returns the backend that ran with the anchors (released)."""
    gamma = _gamma(X)
    ref = _backend(X, "exact", 1, storage, weights)
    want = _epochs(ref, W0, M, gamma, **kw)
    ref.release()
    on = _backend(X, "filtered", 1, storage, weights)
    got_on = _epochs(on, W0, M, gamma, **kw)
    assert on.filter_log[-1][0] == "filtered" and on.filter_log[-1][2] == 0
    state, builds, searches = on.anchor_state, on.anchor_builds, on.anchor_searches
    on.release()
    off = _backend(X, "filtered", 0, storage, weights)
    got_off = _epochs(off, W0, M, gamma, **kw)
    assert off.filter_log[-1][0] == "filtered" and off.anchor_builds == 0 and off.anchor_state == 0
    off.release()
    assert _same(got_on, want), "anchor seeds: not the all-pairs search's results"
    assert _same(got_off, want), "seed pre-pass: not the all-pairs search's results"
    assert _same(got_on, got_off)
    # the buckets were built and compared epochs were seeded from them: all but the pre-pass's one or two reference
    # epochs while the anchors are in use; at least one where the valve dropped them afterwards
    n = kw.get("frozen", 3) + kw.get("evolving", 3)
    assert builds == 1 and state in (1, 2) and searches >= (n - 2 if state == 1 else 1), (builds, state, searches)
    return state


def _map_from(X, M, seed=3):
    return np.asarray(X[np.random.default_rng(seed).choice(X.shape[0], M, replace=False)], dtype=np.float64)


# ---- 1. exactness at the edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float32", "float64", "bf16"])
@pytest.mark.parametrize("N,d,M", [(N, d, M) for N in (1000, 4096) for d in (70, 320) for M in (130, 256)])
def test_exact_with_and_without_anchors(N, d, M, storage):
    X = bench.make_shard_numpy(N, d, 1000 + N + d + M)
    if storage == "float64":
        X = X.astype(np.float64)
    _three_ways(X, _map_from(X, M), M, storage="bf16" if storage == "bf16" else None)


def test_exact_with_zero_sample_weights():
    N, d, M = 4096, 70, 256
    X = bench.make_shard_numpy(N, d, 77)
    w = np.random.default_rng(5).uniform(0.0, 2.0, N)
    w[::3] = 0.0
    _three_ways(X, _map_from(X, M), M, weights=w)


def test_exact_on_isotropic_data_whatever_the_valve_does():
    N, d, M = 4096, 70, 256
    X = bench.make_shard_numpy(N, d, 78, kind="iso")
    state = _three_ways(X, _map_from(X, M), M)
    assert state in (1, 2)


# ---- 2. degenerate anchors ----------------------------------------------------------------------------------------
def test_fewer_samples_than_anchors():
    X = bench.make_shard_numpy(200, 70, 79)
    _three_ways(X, _map_from(X, 130), 130)


def test_every_row_identical():
    rng = np.random.default_rng(80)
    X = np.tile(rng.standard_normal((1, 70)).astype(np.float32), (1000, 1))
    W0 = rng.standard_normal((130, 70))
    _three_ways(X, W0, 130, frozen=3, evolving=1)   # (a map trained on one point degenerates: one evolving epoch)


def test_every_anchor_a_duplicate_of_one_row():
    N = 1024   # anchors: rows 0, 4, 8, ...
    X = bench.make_shard_numpy(N, 70, 81)
    X[::4] = X[0]
    _three_ways(X, _map_from(X[1::4], 130), 130)


def _eight_blobs(seed=82, N=4096, d=320, per=32):
    """Eight well separated clusters and a map laid out cluster by cluster, `per` prototypes each: centres ~100
    apart, points of a cluster ~25 -- the triangle inequality leaves a sample its own cluster's prototypes."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((8, d))
    X = (centres[rng.integers(0, 8, N)] + rng.standard_normal((N, d))).astype(np.float32)
    W0 = np.repeat(centres, per, axis=0) + rng.standard_normal((8 * per, d))
    return X, W0


def _one_epoch_against_exact(X, W0, M, epochs=4):
    gamma, hop = _gamma(X), gi.lattice_hops(*MAPS[M])
    ref = _backend(X, "exact", 1)
    want = ref.epoch(W0, hop, SIGMA, gamma, "compact", True)
    ref.release()
    be = _backend(X, "filtered", 1)
    for _ in range(epochs):   # (the pre-pass's reference epochs first, then the anchors)
        got = be.epoch(W0, hop, SIGMA, gamma, "compact", True)
        assert be.filter_log[-1][0] == "filtered"
        assert np.array_equal(got.winners, want.winners) and np.array_equal(got.distances, want.distances)
        assert np.array_equal(got.new_weights, want.new_weights, equal_nan=True)
    counts, state = be.filter_counts(), be.anchor_state
    be.release()
    return counts, state


def test_exact_on_a_map_with_a_nan_row_and_an_infinite_row():
    """(An infinite row makes max |w|^2 infinite: the pruning form then has no bound for any sample, whatever the
    seeds are, and every list is the whole map -- so this case says nothing about the seeds; the next one does.)"""
    X, W0 = _eight_blobs()
    W0[0] = np.nan          # the first prototype of cluster 0 ...
    W0[32, 5] = np.inf      # ... and of cluster 1
    counts, state = _one_epoch_against_exact(X, W0, 256)
    assert state in (1, 2)


def test_nan_prototypes_are_never_seeds():
    """A seed with a NaN has no bound: its workgroup's list would be the whole map.  NaN rows leave the bounds of the
    other seeds alone (unlike an infinity), so the lists show whether one was chosen."""
    X, W0 = _eight_blobs()
    W0[0] = np.nan
    W0[32, 5] = np.nan
    counts, state = _one_epoch_against_exact(X, W0, 256)
    print("lists with two NaN prototypes: mean %.1f, max %d" % (counts.mean(), counts.max()))
    assert state == 1 and counts.max() < 256 and counts.mean() <= 64


# ---- 3. the per-load state is a function of the samples alone -----------------------------------------------------
def test_state_depends_on_the_samples_only():
    M = 256
    X, W1 = _eight_blobs()
    W2 = _eight_blobs(seed=85)[1]
    gamma, hop = _gamma(X), gi.lattice_hops(*MAPS[M])
    be = _backend(X, "filtered", 1)
    for _ in range(4):   # (the pre-pass's reference epochs; the anchors are in use afterwards)
        be.epoch(W1, hop, SIGMA, gamma, "compact", False)
    assert be.anchor_builds == 1 and be.anchor_state == 1
    runs = []
    for W in (W1, W2, W1):
        r = be.epoch(W, hop, SIGMA, gamma, "compact", True)
        runs.append([(r.winners, r.distances, r.new_weights, r.errors, r.activations, np.array([r.change_total]))])
    assert _same(runs[0], runs[2]) and not _same(runs[0], runs[1])
    assert be.anchor_builds == 1 and be.anchor_state in (1, 2)
    # other samples: the old buckets are gone
    X2, W3 = _eight_blobs(seed=86)
    be.load(X2)
    assert be.anchor_state == 0
    for _ in range(4):
        got = be.epoch(W3, hop, SIGMA, _gamma(X2), "compact", True)
    assert be.anchor_builds == 2 and be.anchor_state in (1, 2)
    be.release()
    ref = _backend(X2, "exact", 1)
    want = ref.epoch(W3, hop, SIGMA, _gamma(X2), "compact", True)
    ref.release()
    assert np.array_equal(got.winners, want.winners) and np.array_equal(got.distances, want.distances)
    assert np.array_equal(got.new_weights, want.new_weights)


# ---- 4. the seeds are worth something -----------------------------------------------------------------------------
def test_lists_stay_at_one_cluster():
    """Mean list length with the anchors <= 64 and <= 1.25 x the pre-pass's.  Measured on MI355X: 39.00 with the
    pre-pass (`anchor_seeds = 0`, the launches of the parent commit: one cluster's 32 prototypes, two clusters' in the
    workgroups that straddle a boundary) and 39.00 with the anchors; a seed kernel that answers the same prototype
    for every anchor leaves the whole map, 256."""
    X, W0 = _eight_blobs()
    gamma, M = _gamma(X), 256
    hop = gi.lattice_hops(*MAPS[M])
    mean = {}
    for anchors in (0, 1):
        be = _backend(X, "filtered", anchors)
        for _ in range(4):
            be.epoch(W0, hop, SIGMA, gamma, "compact", False)
        mean[anchors] = float(be.filter_counts().mean())
        assert be.anchor_state == anchors
        be.release()
    print("mean list length: pre-pass %.2f, anchors %.2f" % (mean[0], mean[1]))
    assert mean[1] <= 64.0 and mean[1] <= 1.25 * mean[0]


def test_lists_stay_at_one_cluster_when_tiles_span_the_clusters():
    """The same eight clusters with prototype j in cluster j % 8: every 16-prototype tile of the anchor-seed kernel now
    holds two prototypes of each cluster, so a seed that is the wrong prototype of the right tile lies in another
    cluster and its workgroup's list takes that cluster in.  Renumbering the prototypes changes neither the buckets
    nor the geometry: the lists are as long as on the map laid out cluster by cluster."""
    X, W0 = _eight_blobs()
    gamma, M = _gamma(X), 256
    hop = gi.lattice_hops(*MAPS[M])
    j = np.arange(M)
    Wp = np.ascontiguousarray(W0[(j % 8) * 32 + j // 8])
    assert np.array_equal(np.sort(Wp, axis=0), np.sort(W0, axis=0)) and np.array_equal(Wp[8], W0[1])
    mean = {}
    for name, W in (("by cluster", W0), ("interleaved", Wp)):
        be = _backend(X, "filtered", 1)
        for _ in range(4):
            be.epoch(W, hop, SIGMA, gamma, "compact", False)
        mean[name] = float(be.filter_counts().mean())
        assert be.anchor_state == 1 and be.anchor_searches >= 1
        be.release()
    print("mean list length with the anchors: by cluster %.2f, interleaved %.2f" % (mean["by cluster"], mean["interleaved"]))
    assert mean["interleaved"] <= 64.0 and mean["interleaved"] <= 1.25 * mean["by cluster"]
